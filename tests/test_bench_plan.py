"""Pre-flight of bench.py's plan (CPU): the block pool a bench run is given must hold every block the run can reach,
for every (steps, warmup) a driver may pass and however many regions the box's speed makes the run time.

Round 2's driver bench died in exactly this gap: the c5 robot drove in a straight line forever, the default pool held
about 157 updates, `--steps 20 --warmup 5` needed 165, and only `--steps 10 --warmup 3` had ever been run."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402
from gie import scenes, tiling  # noqa: E402

COMMANDS = [(10, 3), (20, 5), (50, 10), (100, 20), (1, 0)]


def blocks_reached(size, voxel, updates, tile_off=(0, 0, 0), ghost=0):
    """Bounding box, in 8x8x8 blocks, of everything the c5 volume (+ `ghost` voxels around it) overlaps in `updates` frames."""
    lo = np.full(3, 1 << 30)
    hi = np.full(3, -(1 << 30))
    for i in range(updates):
        pos, _ = bench.c5_pose(scenes, i, voxel)
        pvt = np.array(scenes.local_pivot(pos, voxel, size, tile_off))
        lo = np.minimum(lo, (pvt - ghost) >> 3)
        hi = np.maximum(hi, (pvt + np.array(size) - 1 + ghost) >> 3)
    return int(np.prod(hi - lo + 1))


@pytest.mark.parametrize("steps,warmup", COMMANDS)
@pytest.mark.parametrize("world", [1, 8])
def test_pool_holds_every_frame_the_command_can_reach(steps, warmup, world):
    size, voxel = (512, 512, 512), 0.05
    # the slowest plausible box times ONE region (>= 0.5 s), the fastest all MAX_REGIONS of them: plan for the latter
    updates = bench.planned_updates(warmup, steps)
    assert updates == warmup + steps * bench.MAX_REGIONS + steps
    pool = bench.pool_blocks("c5", size, updates)
    assert 0 < pool <= 4000000
    for rank in range(world):
        off = tiling.tile_offset_voxels(rank, world, size) if world > 1 else (0, 0, 0)
        need = blocks_reached(size, voxel, updates, off, ghost=1 if world > 1 else 0)
        assert need <= pool, "rank %d: %d blocks reached, pool %d" % (rank, need, pool)


def test_c5_drive_is_bounded():
    """Out and back: frame 2 * C5_TURN stands where frame 0 stood, and no frame is farther out than C5_TURN steps."""
    xs = [float(bench.c5_pose(scenes, i, 0.05)[0][0]) for i in range(5 * bench.C5_TURN)]
    assert xs[0] == xs[2 * bench.C5_TURN] == xs[4 * bench.C5_TURN] == 0.0
    assert max(xs) == pytest.approx(bench.C5_TURN * bench.C5["delta_vox"] * 0.05)
    assert min(xs) == 0.0
    # consecutive frames are exactly delta_vox voxels apart (the volume moves every frame: waves are seeded every step)
    d = np.abs(np.diff(np.array(xs))) / 0.05
    assert np.allclose(d, bench.C5["delta_vox"], atol=1e-3)


def test_small_volume_runs_the_whole_plan_on_the_planned_pool(oracle_lib):
    """The driver's command (--steps 20 --warmup 5) at its worst case of 12 regions, replayed at 32^3 through the sequential
    emulation of the device logic on a pool sized by the same rule: no capacity error, and the map holds exactly the blocks the plan counted."""
    import gie
    from emu_py import EmuMapper
    size, voxel = (32, 32, 32), 0.05
    updates = bench.planned_updates(5, 20)
    pool = bench.pool_blocks("c5", size, updates) - 4096      # without the fixed margin: the rule itself has to hold
    cfg = gie.make_config(voxel, size, cutoff_dist=0.5, fast_mode=False, max_blocks=pool)
    m = EmuMapper(cfg)
    for i in range(updates):
        pos, q = bench.c5_pose(scenes, i, voxel)
        lab = scenes.hash_world_labels(scenes.local_pivot(pos, voxel, size), size, i, seed=5, p_occ=0.01, toggle_frac=0.25)
        m.update(pos, q, "labels", lab.astype(np.int8))
        if i % 16 == 0:
            m.sync()                      # raises on a capacity error
    m.sync()
    used = m.stats()["blocks_total"]
    assert used <= pool
    assert used == blocks_reached(size, voxel, updates)       # full observation: every block the volume ever overlapped exists
    m.close()


def test_failure_still_prints_one_json_line(tmp_path):
    """Without a GPU bench.py cannot run: it must still print exactly one JSON line carrying an "error" key."""
    import json
    import subprocess
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "2", "--warmup", "1"], capture_output=True, text=True,
                       env=dict(os.environ, HIP_VISIBLE_DEVICES="", CUDA_VISIBLE_DEVICES=""), timeout=300)
    lines = [l for l in p.stdout.splitlines() if l.strip().startswith("{")]
    assert p.returncode != 0
    assert len(lines) == 1
    j = json.loads(lines[0])
    assert "error" in j and j["value"] is None


def _canned_result(preset, ms, big=True):
    """What run_workload returns, with canned numbers (and, big=True, the per-kernel trees that broke round 4's line)."""
    names = ["mark_commit", "edt_pass_z", "edt_pass_x", "fuse", "frontiers", "waves", "edt_pass_y", "ogm_classify", "block_alloc", "edt_prep",
             "ray_free", "ray_register"]
    sweeps = {k: {"avg_launch_ms": 0.7674, "achieved": 4459.3, "frac": 0.5574, "frac_basis": "pmc", "traffic": 3422079359, "achieved_algorithmic": 12243.1,
                  "frac_algorithmic": 1.5304, "alg_bytes_per_launch": 9395240960, "layout_bytes_per_launch": 2818572288, "alg_bytes_per_voxel": 70,
                  "layout_bytes_per_voxel": 21, "voxels_per_launch": 134217728} for k in names}
    roof = dict(sweeps["mark_commit"], bound="hbm", kernel="mark_commit", peak=8000.0, unit="GB/s", csrc_hash="505f8d90a20d65cf",
                traffic_source="profiles/r05_c5_hbm_traffic.txt: " + "x" * 400, note="n" * 1500)
    p = bench.PRESETS[preset]
    return {"value": 57611.3, "ms_per_step": ms, "hz": 429.2, "steps": 20, "warmup": 5, "timed_regions": 11, "region_ms": [46.6] * 11, "timed_s": 0.513,
            "step_ms": {"median": 2.31, "p95": 2.36, "min": 2.29, "max": 2.4, "n": 20, "how": "h" * 100},
            "config": {"workload": "%dx%dx%d @ %.2f m, %s" % (p["size"] + (p["voxel"], "w" * 200)), "preset": preset, "baseline_config": bench.BASELINE_CONFIG.get(preset),
                       "grid": list(p["size"]), "voxel_m": p["voxel"], "cutoff_m": p["cutoff"], "fast_mode": p["fast"], "drive": {"mode": "turn"},
                       "tiles": "single volume", "known_voxel_fraction": 1.0, "wave_visits_per_step": [1234.5, 23456.7, 56789.1],
                       "wave_levels_last_step": [3, 9, 12], "blocks": 313344},
            "kernels_ms_per_step": {k: 0.7674 for k in names}, "ms_per_step_instrumented": 2.45,
            "roofline": roof, "roofline_wavefront_sweep": {"kernels": names[:3], "ms_per_step": 1.2, "frac": 0.44, "frac_basis": "pmc", "frac_algorithmic": 0.95,
                                                            "per_kernel_ms": {k: 0.1 for k in names}},
            "roofline_update": {"ms_per_step": ms, "frac": 0.42, "frac_basis": "pmc", "frac_algorithmic": 0.89, "note": "n" * 300},
            "roofline_sweeps": sweeps if big else {}}


def test_bench_line_stays_below_8_kb_and_round_trips():
    """VERDICT r4 'next' #1: the ONE line on stdout is the driver's record (BENCH_r04.parsed was null: a 21.8 KB line).  The line
    builder on canned numbers — every default extra run with full per-kernel trees, the cpu baseline, an accuracy object — must
    give < 8 KB of JSON that parses back, carries the contract's keys, and holds no string above 120 characters; the rest goes to
    the side file it names."""
    import json
    main_res = _canned_result("c5", 2.3298)
    main_res["accuracy"] = {"rms_m": 0.0123, "max_err_m": 0.2, "edt_less": 12, "edt_more": 0, "voxels": 134217728, "how": "h" * 300}
    extras = {wl: _canned_result(wl, 0.4507) for wl in bench.DEFAULT_EXTRAS}
    cpu = {"value": 192.3, "unit": "Mvoxels/s", "cores": 256, "host_cores": 256, "kind": "port", "stage": "s" * 200, "ms_per_update": 698.0, "sample": "p" * 200,
           "full_update_1core": {"value": 10.2, "unit": "Mvoxels/s", "cores": 1, "kind": "port", "stage": "t" * 150, "sample": "q" * 200}}
    line, full = bench.build_line(main_res, extras, cpu, 1)
    text = json.dumps(line)
    assert len(text) < 8192, len(text)
    back = json.loads(text)
    assert back == line
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config",
              "roofline", "cpu_baseline", "ms_per_step_by_workload", "frac_by_workload", "detail"):
        assert k in back, k
    assert back["steps"] == 20 and back["warmup"] == 5 and back["n_gpus"] == 1 and back["vs_baseline"] is None
    for k in ("bound", "achieved", "peak", "unit", "frac", "traffic", "kernel", "avg_launch_ms"):
        assert k in back["roofline"], k
    for k in ("value", "unit", "cores", "kind", "sample"):
        assert k in back["cpu_baseline"], k
    assert set(back["ms_per_step_by_workload"]) == {"c5"} | set(bench.DEFAULT_EXTRAS)
    assert {"c2", "c3", "c4"} <= set(back["ms_per_step_by_workload"])            # BASELINE configs 2 / 3 / 4 are timed by default (VERDICT r4 'missing' #1)

    def strings(o):
        if isinstance(o, dict):
            for v in o.values():
                yield from strings(v)
        elif isinstance(o, list):
            for v in o:
                yield from strings(v)
        elif isinstance(o, str):
            yield o
    assert max(len(t) for t in strings(back)) <= 120
    # nothing is lost: the side file has the per-kernel trees of every run and the long notes
    assert full["extra_runs"]["c3"]["roofline_sweeps"]["edt_pass_z"]["traffic"] == 3422079359
    assert "roofline" in full["notes"] and full["roofline"]["note"]
    # a tiled run's line (no extras, no cpu baseline) carries the exchange it timed
    tiled = _canned_result("c5", 2.9, big=False)
    tiled["config"].update({"tiles": "2x2x2 tiles of 512x512x512, one per GPU", "exchange": "RCCL", "rccl_ranks": 8, "halo_mode": "converged",
                            "halo_max_rounds": bench.HALO_MAX_ROUNDS, "rounds_per_update": 2.25, "updates_unconverged": 0, "exchange_notes": []})
    l8, _ = bench.build_line(tiled, {}, None, 8)
    assert l8["n_gpus"] == 8 and l8["config"]["rounds_per_update"] == 2.25 and l8["config"]["rccl_ranks"] == 8 and l8["config"]["updates_unconverged"] == 0
    assert len(json.dumps(l8)) < 8192


def test_plain_line_is_the_headline():
    """A plain run (no --full) times the headline only: its line carries the contract's keys and nothing of the instrumented
    replay, the other workloads or the side file."""
    import json
    main_res = _canned_result("c5", 2.3298, big=False)
    for k in ("step_ms", "kernels_ms_per_step", "ms_per_step_instrumented", "roofline", "roofline_wavefront_sweep", "roofline_update", "roofline_sweeps"):
        del main_res[k]
    del main_res["config"]["known_voxel_fraction"]
    line, _ = bench.build_line(main_res, {}, None, 1, full_file=None)
    back = json.loads(json.dumps(line))
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup", "config"):
        assert k in back, k
    assert back["ms_per_step"] == 2.3298 and back["higher_is_better"] is True and back["unit"] == "Mvoxels/s"
    for k in ("roofline", "kernels_ms_per_step", "cpu_baseline", "ms_per_step_by_workload", "detail"):
        assert k not in back, k


def test_hash_world_planes_depend_on_pivot_and_parity_only(monkeypatch):
    """HashWorldFeed keeps one label plane per (pivot, frame parity): each frame's plane must be the one its own frame index gives,
    and a long region of the out-and-back drive must need no more than C5_TURN + 1 planes."""
    import torch
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **k: None)
    size, voxel = (24, 16, 8), 0.05
    feed = bench.HashWorldFeed(torch, scenes, torch.device("cpu"), voxel, size, (0, 0, 0))
    first, count = 5, 4 * bench.C5_TURN + 3
    feed.prepare(first, count)
    assert len(feed.planes) <= bench.C5_TURN + 1
    by_ptr = {t.data_ptr(): t for t in feed.planes.values()}
    for i in range(first, first + count):
        pos, _ = bench.c5_pose(scenes, i, voxel)
        want = scenes.hash_world_labels(scenes.local_pivot(pos, voxel, size), size, i, seed=bench.C5["seed"], p_occ=bench.C5["p_occ"],
                                        toggle_frac=bench.C5["toggle_frac"])
        assert np.array_equal(by_ptr[feed.ptrs[i]].numpy(), want.astype(np.int8)), i
    feed.prepare(0, 2)                       # a later region drops the planes it does not need
    assert len(feed.planes) == 2


def test_dump_sample_is_fixed_and_small():
    """--dump-outputs: a volume above DUMP_SAMPLE voxels is written at a fixed, seeded, sorted sample; all files <= 64 MB."""
    n = 512 ** 3
    idx = bench.dump_sample_index(n)
    assert idx.shape == (bench.DUMP_SAMPLE,) and np.all(np.diff(idx) > 0) and idx[0] >= 0 and idx[-1] < n
    assert np.array_equal(idx, bench.dump_sample_index(n))
    assert bench.dump_sample_index(bench.DUMP_SAMPLE) is None
    # edt f32 + type f32 + dist_sq f64 + coc 3 x f64 + sample_index f64 per voxel
    assert bench.DUMP_SAMPLE * (4 + 4 + 8 + 24 + 8) <= 64 * 2 ** 20


def test_presets_are_the_baseline_configs():
    """BASELINE.json configs 2-5 as bench presets, with the reference's parameters (cfg/cow_lady_params.yaml:15-27,
    cfg/ugv_laser3D_params.yaml:17-28, cfg/uav_laser3D_params.yaml:16-28 + launch/uav_raycast.launch:4-8)."""
    P = bench.PRESETS
    assert P["c5"]["size"] == (512, 512, 512) and P["c5"]["voxel"] == 0.05 and P["c5"]["cutoff"] == 2.0 and not P["c5"]["fast"]
    for k in ("c2", "c2_projective"):
        assert P[k]["size"] == (256, 256, 256) and P[k]["voxel"] == 0.05 and P[k]["cutoff"] == 2.0 and not P[k]["fast"] and P[k]["feed"] == "depth"
    assert not P["c2"]["projective"] and P["c2_projective"]["projective"]
    assert (bench.DEPTH_CAM["cols"], bench.DEPTH_CAM["rows"]) == (640, 480) and bench.DEPTH_CAM["cols"] * bench.DEPTH_CAM["rows"] == 307200
    for k in ("c3", "c3_projective"):
        assert P[k]["size"] == (512, 512, 512) and P[k]["voxel"] == 0.1 and P[k]["cutoff"] == 100.0 and not P[k]["fast"]
    assert bench.LIDARS[P["c3"]["sensor"]][4] is None and bench.LIDARS[P["c3_projective"]["sensor"]][4] == 440
    for k in ("c4", "c4_nofast"):
        assert P[k]["size"] == (320, 320, 40) and P[k]["voxel"] == 0.05 and P[k]["cutoff"] == 5.0 and bench.LIDARS[P[k]["sensor"]][4] is None
    assert P["c4"]["fast"] and not P["c4_nofast"]["fast"]
    import gie
    for k, want in (("c2", 1600), ("c4", 10000), ("c3", 1000000)):          # cutoff in voxels², SURVEY 8 config shorthands
        assert gie.make_config(P[k]["voxel"], P[k]["size"], cutoff_dist=P[k]["cutoff"]).cutoff_grids_sq == want


def test_dominant_kernel_is_a_kernel_not_a_stage_of_several_launches():
    """bench.dominant_stage: `waves` is two launches — on the headline their sum is as long as pass X, each of them is shorter"""
    import bench
    headline = {"edt_pass_x": (0.2612 * 20, 20), "waves": (0.2617 * 20, 20), "edt_pass_z": (0.26 * 20, 20), "mark_commit": (0.12 * 20, 20), "block_alloc": (0.13 * 20, 20)}
    assert bench.dominant_stage(headline) == "edt_pass_x"
    flood = {"edt_pass_x": (0.11 * 10, 10), "waves": (1.2 * 10, 10), "ogm_classify": (0.245 * 10, 10)}      # waves A / B alone are most of the update
    assert bench.dominant_stage(flood) == "waves"
    assert bench.dominant_stage({"fuse": (1.0, 4), "frontiers": (1.9, 4)}) == "fuse"
