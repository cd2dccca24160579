"""GPU parity: libgie_hip.so (HIP kernels on the MI355X) against the CPU oracle through the
C-ABI, every stage of every frame bit-exact (float EDT within 1e-6 relative)."""
import numpy as np
import pytest

import gie
import parity
from oracle_py import OracleMapper, brute_force_edt

pytestmark = pytest.mark.gpu

SCENARIOS = [
    parity.Scenario("depth", (48, 40, 24), sensor="depth", frames=14, delta_vox=5, yaw_deg=47.0),
    parity.Scenario("raycast", (40, 40, 20), sensor="pointcloud", frames=12, delta_vox=5, yaw_deg=47.0),
    parity.Scenario("vlp16", (48, 48, 16), sensor="multiscan", frames=12, delta_vox=5, yaw_deg=10.0),
    # a volume tall enough for most of it to lie above / below the lidar's field of view: the box test of the multiscan OGM (round 6)
    parity.Scenario("vlp16_tall", (64, 56, 72), voxel=0.05, sensor="multiscan", frames=5, delta_vox=4, yaw_deg=25.0, extent=(2.5, 2.5, 2.0)),
    parity.Scenario("scan2d", (40, 40, 8), sensor="scan2d", frames=6, delta_vox=3, yaw_deg=10.0),
    parity.Scenario("mixed", (48, 40, 24), sensor="mixed", frames=12, delta_vox=5, yaw_deg=47.0),
    parity.Scenario("fast_mode", (48, 40, 24), sensor="mixed", frames=12, delta_vox=5, yaw_deg=47.0, fast_mode=True),
    parity.Scenario("planner_boxes", (40, 40, 24), sensor="mixed", frames=9, delta_vox=4, yaw_deg=30.0,
                    for_motion_planner=True, ext_boxes=True, min_h=-0.8, max_h=1.0),
    parity.Scenario("cutoff_small", (32, 32, 16), sensor="lidar_points", frames=12, delta_vox=6, yaw_deg=5.0,
                    cutoff_dist=0.5),
    parity.Scenario("odd_dims", (37, 29, 11), sensor="mixed", frames=9, delta_vox=3, yaw_deg=33.0),
    parity.Scenario("flat_2d", (40, 40, 1), sensor="scan2d", frames=5, delta_vox=3, yaw_deg=10.0),
    # ray casting in thin volumes: rays cut by the maximum length 0.707*X*w (X = 16), and rays that leave the volume long before they end
    parity.Scenario("thin_x", (16, 200, 8), sensor="lidar_points", frames=6, delta_vox=5, yaw_deg=40.0, lidar_az=720),
    parity.Scenario("thin_y", (200, 16, 8), sensor="lidar_points", frames=6, delta_vox=5, yaw_deg=40.0, lidar_az=720),
    # a volume taller than 512 voxels: more than 64 z tiles per tile column (the upper tiles were never listed nor flagged)
    parity.Scenario("tall_z", (16, 24, 600), voxel=0.05, sensor="labels", frames=4, delta_vox=5, yaw_deg=2.0, seed=8, cutoff_dist=1.0, p_occ=0.004),
    # BASELINE C3's wave parameters (ugv yaml: cutoff 100 m => no cutoff at all, full waves A+B), small volume
    parity.Scenario("c3_no_cutoff", (56, 56, 20), voxel=0.1, sensor="multiscan", frames=10, delta_vox=6, yaw_deg=12.0,
                    cutoff_dist=100.0, extent=(5.0, 5.0, 1.5)),
    # BASELINE C1: 32^3 dense grid, one point-cloud frame
    parity.Scenario("c1_32cube", (32, 32, 32), voxel=0.05, sensor="lidar_points", frames=1, delta_vox=0, yaw_deg=0.0,
                    extent=(0.7, 0.7, 0.7), n_boxes=12),
    # larger volumes: every EDT template (CP=2,4,8) and multi-block sweeps
    parity.Scenario("mid_128", (128, 96, 64), voxel=0.05, sensor="mixed", frames=8, delta_vox=6, yaw_deg=25.0,
                    extent=(3.0, 3.0, 1.2), img=(240, 320, 260.0)),
    parity.Scenario("c4_slab", (320, 320, 40), voxel=0.05, sensor="lidar_points", frames=5, delta_vox=4, yaw_deg=2.0,
                    extent=(8.0, 8.0, 1.0), n_boxes=60, cutoff_dist=5.0, lidar_az=900),
    # BASELINE C4 as SURVEY §8(d) states it: the same volume with fast_mode = true (cfg/uav_laser3D_params.yaml:27)
    parity.Scenario("c4_slab_fast", (320, 320, 40), voxel=0.05, sensor="lidar_points", frames=5, delta_vox=4, yaw_deg=2.0,
                    extent=(8.0, 8.0, 1.0), n_boxes=60, cutoff_dist=5.0, lidar_az=900, fast_mode=True),
    # BASELINE C5's sensor-less world through gie_ogm_labels (vector kernel: X % 16 == 0; functor path: odd sizes / robot sphere)
    parity.Scenario("c5_hash_world", (48, 48, 32), voxel=0.05, sensor="labels", frames=8, delta_vox=8, yaw_deg=2.0, seed=5,
                    cutoff_dist=2.0, p_occ=0.01),
    parity.Scenario("c5_dense_odd", (40, 36, 20), voxel=0.05, sensor="labels", frames=8, delta_vox=3, yaw_deg=2.0, seed=6,
                    cutoff_dist=0.5, p_occ=0.05, toggle=0.5),
    parity.Scenario("c5_planner", (64, 48, 24), voxel=0.05, sensor="labels", frames=5, delta_vox=5, yaw_deg=2.0, seed=7,
                    cutoff_dist=1.0, p_occ=0.02, for_motion_planner=True),
    parity.Scenario("c5_128cube", (128, 128, 128), voxel=0.05, sensor="labels", frames=5, delta_vox=8, yaw_deg=2.0, seed=5,
                    cutoff_dist=2.0, p_occ=0.01),
    parity.Scenario("c2_256cube", (256, 256, 256), voxel=0.05, sensor="mixed", frames=4, delta_vox=4, yaw_deg=2.0,
                    extent=(6.0, 6.0, 3.0), n_boxes=60, img=(480, 640, 525.0)),
    # block-pool lifecycle (gie_config.retain_radius_blocks): see tests/test_host_logic.py
    parity.Scenario("retain_c5_out_and_back", (32, 32, 16), voxel=0.05, sensor="labels", frames=26, delta_vox=8, yaw_deg=2.0, seed=5,
                    cutoff_dist=1.0, p_occ=0.01, retain=2, turn=9, probe_margin=60),
    # obstacle-free scans in between, on the move: known voxels that are not committed (EMPTY pairs) while their stored pair is
    # still owed from an earlier update of the same stay in the volume (gie_commit_pair / gie_pair_flush_voxel)
    parity.Scenario("blink_empty_scans", (32, 28, 12), voxel=0.05, sensor="labels_blink", frames=18, delta_vox=5, yaw_deg=2.0, seed=9,
                    cutoff_dist=1.0, p_occ=0.004, toggle=0.3, probe_margin=30),
    parity.Scenario("retain_lidar", (48, 48, 16), sensor="multiscan", frames=16, delta_vox=7, yaw_deg=10.0, retain=1, probe_margin=40),
    # a robot that turns round and meets the blocks it has erased again (round-4 fuzz, seed 51 #30 and seed 53 #57: the table of the
    # fuse before reaches a cell beyond the retention box and used to hand an erased block on from update to update)
    parity.Scenario("retain_turn_back", (72, 64, 96), voxel=0.1, sensor="mixed", frames=10, delta_vox=8, yaw_deg=28.425771268056188, seed=870,
                    cutoff_dist=0.5, extent=(6.76, 6.76, 4.34), toggle=0.25, lidar_az=180, p_occ=0.003, retain=1, turn=3),
    parity.Scenario("retain_turn_back_lidar", (152, 96, 160), voxel=0.1, sensor="lidar_points", frames=10, delta_vox=5, yaw_deg=7.861227329719755, seed=841,
                    cutoff_dist=0.5, extent=(10.6, 10.6, 6.9), toggle=0.5, lidar_az=720, p_occ=0.003, retain=1, turn=3, probe_margin=40),
    parity.Scenario("retain_odd_r1", (37, 29, 11), sensor="mixed", frames=12, delta_vox=5, yaw_deg=33.0, retain=1, turn=5, probe_margin=40),
    # wave C, round 0, across a tile border: the neighbour is a seed that wave B left on an UNKNOWN face voxel — accepted against the
    # batch distance (wave_core.cuh:334), above the stale pair the plane still holds for it — and a proposal between the two used to
    # be dropped by the pre-read of the halo (round-4 fuzz, --focus retain --big, seed 83 #63: one voxel, 182 instead of 179)
    parity.Scenario("wave_c_seed_above_stale_pair", (96, 120, 160), voxel=0.2, sensor="mixed", frames=11, delta_vox=10, yaw_deg=30.029303880177924,
                    seed=742, cutoff_dist=100.0, extent=(20.2, 20.2, 13.3), toggle=0.5, lidar_az=360, p_occ=0.01, retain=2, turn=5, probe_margin=40),
]


@pytest.mark.parametrize("sc", SCENARIOS, ids=[s.name for s in SCENARIOS])
def test_hip_matches_oracle(oracle_lib, sc):
    parity.run_and_compare(sc, OracleMapper, gie.Mapper)


@pytest.mark.parametrize("sc", parity.UNEVEN_DRIVES, ids=[s.name for s in parity.UNEVEN_DRIVES])
@pytest.mark.parametrize("production", [False, True], ids=["staged", "production"])
def test_uneven_drives_catch_up_the_deferred_records(oracle_lib, sc, production):
    """drives that change speed and direction in volumes whose sides are no multiples of 8 (parity.UNEVEN_DRIVES)."""
    parity.run_and_compare(sc, OracleMapper, gie.Mapper, production=production)


def test_voxel_addresses_beyond_2_to_31(oracle_lib, monkeypatch):
    """voxel addresses (slot * 512 + index) are 64-bit.  A pool of 4.3 M blocks (84 GB of planes on the device) whose
    slots are handed out from 4.25 M on (GIE_DEBUG_POOL_BASE): every address of the run lies beyond 2^31.  Slot numbers are not
    observable, so the run has to equal the oracle's like any other — the hash world with waves A / B / C (every kernel that
    forms an address: allocation, block initialisation, fuse, Mark + commit, obtainFrontiers, the block rounds, the pair flush,
    global queries) and a lidar scene through ray casting and the projective OGM."""
    monkeypatch.setenv("GIE_DEBUG_POOL_BASE", "4250000")
    from hooks_py import HooksMapper                   # the switch exists in the test build of the library only

    def big_pool(cfg):
        big = type(cfg).from_buffer_copy(cfg)
        big.max_blocks = 4300000
        try:
            return HooksMapper(big)
        except RuntimeError as e:
            if "allocation failed" in str(e):
                pytest.skip("the device cannot hold an 84 GB block pool right now")
            raise

    for name in ("c5_hash_world", "mixed", "raycast"):
        sc = [x for x in SCENARIOS if x.name == name][0]
        parity.run_and_compare(sc, OracleMapper, big_pool)


def test_long_drive_on_a_fixed_pool(oracle_lib):
    """a 2 000-update C5 drive in a straight line at 64^3 on a FIXED pool (retain_radius_blocks = 2: the pool holds
    the retention zone, 13^3 blocks, and nothing more — without recycling the drive would need 130 000 blocks).  HIP == oracle:
    the local volume every 50 updates, global probes reaching past the retention zone, and the live block count; the hash table
    goes through 31 rebuilds on the way."""
    from gie import scenes
    size, voxel, R = (64, 64, 64), 0.05, 2
    cfg = gie.make_config(voxel, size, cutoff_dist=1.0, fast_mode=False, retain_radius_blocks=R, max_blocks=13 ** 3)
    a, b = OracleMapper(cfg), gie.Mapper(cfg)
    rng = np.random.default_rng(12)
    try:
        for i in range(2000):
            pos, q = scenes.pose(i, voxel, delta_vox=8, yaw_deg=1.0)
            lab = scenes.hash_world_labels(scenes.local_pivot(pos, voxel, size), size, i, seed=5, p_occ=0.01, toggle_frac=0.25).astype(np.int8)
            for m in (a, b):
                m.update(pos, q, "labels", lab)
            if i % 50 == 0 or i == 1999:
                ra, rb = a.read_local(), b.read_local()
                for key in ("type", "dist_sq", "coc"):
                    assert np.array_equal(ra[key], rb[key]), (i, key)
                xyz = parity.probe_coords(a.pivot(), size, rng, n=6000, margin=64)
                ga, gb = a.query_global(xyz), b.query_global(xyz)
                for key in ("occ_val", "vox_type", "dist_sq", "coc"):
                    assert np.array_equal(ga[key], gb[key]), (i, key)
                sa, sb = a.stats(), b.stats()
                for key in ("blocks_total", "visits_a", "visits_b", "visits_c"):
                    assert sa[key] == sb[key], (i, key, sa[key], sb[key])
                assert sb["blocks_total"] <= 13 ** 3
    finally:
        a.close()
        b.close()


@pytest.mark.parametrize("shape,dens,seed", [
    ((64, 64, 64), 0.001, 1), ((100, 70, 33), 0.01, 2), ((130, 20, 257), 0.0005, 3), ((16, 300, 16), 0.02, 4),
    ((512, 8, 8), 0.003, 5), ((8, 8, 512), 0.003, 6), ((8, 512, 8), 0.003, 7), ((65, 129, 1), 0.01, 8),
    ((1, 1, 1), 1.0, 9), ((40, 40, 40), 1.0, 10),
    # the 1024-long axis templates: envelope passes with CP = 16; pass Y along 1024 rows, which at X = 16 (a multiple of 4) is
    # k_edt_y4<32> — the 32-mask-word kernel k_edt_y<32,16> takes Y > 512 only where X % 4 != 0 (test_edt_forms_gpu.py: y_7x513,
    # y_67x1024, y_3x1024)
    ((1024, 16, 12), 0.002, 11), ((16, 1024, 12), 0.002, 12), ((12, 16, 1024), 0.002, 13),
    # pass Z picks its argmin form by the number of planes with obstacles: banded (<= 160) or divide & conquer
    ((8, 8, 1000), 0.001, 14), ((24, 24, 400), 0.02, 15), ((20, 20, 200), 0.05, 16), ((16, 16, 130), 0.003, 17),
    # pass X the same way by the number of obstacle columns of a plane: divide & conquer with more sites than half the
    # wave's site list (they overwrite the banded form's linear records, which live there), with fewer, and banded rows
    ((512, 24, 8), 0.05, 18), ((320, 16, 8), 0.08, 19), ((512, 12, 6), 0.01, 20), ((1024, 12, 4), 0.06, 21),
])
def test_batch_edt_random_grids(oracle_lib, shape, dens, seed):
    """EDT passes alone on random obstacle fields, through the full C-ABI: types are injected
    by a point cloud (one point per obstacle voxel centre, sensor at a far corner so no ray
    crosses the volume... simpler: compare HIP with the oracle, and the oracle with brute force
    where the grid is small enough)."""
    X, Y, Z = shape
    rng = np.random.default_rng(seed)
    occ = rng.random((Z, Y, X)) < dens
    occ[Z // 2, Y // 2, X // 2] = True
    w = 0.1
    cfg = gie.make_config(w, shape, cutoff_dist=1.0)
    zz, yy, xx = np.nonzero(occ)
    a, b = OracleMapper(cfg), gie.Mapper(cfg)
    try:
        pos = (0.0, 0.0, 0.0)
        for m in (a, b):
            m.set_pose(pos)
        pv = np.array(a.pivot())
        pts = ((np.stack([xx, yy, zz], -1) + pv) * np.float32(w)).astype(np.float32)
        for m in (a, b):
            m.ogm_pointcloud(pts)
            m.fuse()
            m.batch_edt()
        ea, eb = a.read_batch_edt(), b.read_batch_edt()
        assert np.array_equal(ea["dist_sq"], eb["dist_sq"])
        assert np.array_equal(ea["coc"], eb["coc"])
        ta = a.read_local(edt=False, dist_sq=False, coc=False)["type"]
        if X * Y * Z <= 300000:
            bf = brute_force_edt((ta == 2).astype(np.int8))
            assert np.array_equal(eb["dist_sq"], bf)
    finally:
        a.close()
        b.close()


def _edt_pair(shape, occ):
    """Batch EDT of an occupancy grid through oracle and HIP (types injected by one point per obstacle voxel)."""
    X, Y, Z = shape
    w = 0.1
    cfg = gie.make_config(w, shape, cutoff_dist=1.0)
    zz, yy, xx = np.nonzero(occ)
    a, b = OracleMapper(cfg), gie.Mapper(cfg)
    try:
        for m in (a, b):
            m.set_pose((0.0, 0.0, 0.0))
        pv = np.array(a.pivot())
        pts = ((np.stack([xx, yy, zz], -1) + pv) * np.float32(w)).astype(np.float32)
        for m in (a, b):
            m.ogm_pointcloud(pts)
            m.fuse()
            m.batch_edt()
        return a.read_batch_edt(), b.read_batch_edt()
    finally:
        a.close()
        b.close()


@pytest.mark.parametrize("shape,dens,gap,seed", [
    # dense rows / columns take the windowed form of passes X and Z (most sites real); a wide empty stretch inside a
    # dense row makes the window give up and the envelope forms take over — both sides of that switch, every template
    ((256, 200, 8), 0.01, None, 31), ((512, 64, 4), 0.3, None, 32), ((16, 16, 512), 0.01, None, 33), ((24, 20, 300), 0.2, None, 34),
    ((512, 40, 6), 0.05, ("x", 120, 400), 35), ((12, 12, 512), 0.05, ("z", 100, 330), 36), ((320, 48, 8), 0.04, ("x", 10, 150), 37),
    ((1024, 24, 4), 0.1, ("x", 300, 340), 38), ((8, 24, 1024), 0.1, ("z", 500, 600), 39), ((512, 512, 2), 0.01, None, 40),
])
def test_batch_edt_dense_rows(oracle_lib, shape, dens, gap, seed):
    X, Y, Z = shape
    rng = np.random.default_rng(seed)
    occ = rng.random((Z, Y, X)) < dens
    if gap is not None:
        ax, lo, hi = gap
        if ax == "x":
            occ[:, :, lo:hi] = False
        else:
            occ[lo:hi, :, :] = False
    occ[0, 0, 0] = True
    ea, eb = _edt_pair(shape, occ)
    assert np.array_equal(ea["dist_sq"], eb["dist_sq"])
    assert np.array_equal(ea["coc"], eb["coc"])


def test_empty_volume(oracle_lib):
    cfg = gie.make_config(0.1, (24, 20, 12))
    a, b = OracleMapper(cfg), gie.Mapper(cfg)
    try:
        for m in (a, b):
            m.set_pose((0.0, 0.0, 0.0))
            m.ogm_pointcloud(np.zeros((0, 3), np.float32))
            m.fuse(); m.batch_edt(); m.merge()
        ea, eb = a.read_batch_edt(), b.read_batch_edt()
        assert np.array_equal(ea["coc"], eb["coc"]) and (eb["coc"] == -1).all()
        ra, rb = a.read_local(), b.read_local()
        for k in ("type", "dist_sq", "coc", "edt"):
            assert np.array_equal(ra[k], rb[k])
    finally:
        a.close(); b.close()


def test_costmap_payload(oracle_lib):
    sc = parity.Scenario("cm", (32, 32, 16), sensor="depth", frames=2)
    cfg = sc.config()
    a, b = OracleMapper(cfg), gie.Mapper(cfg)
    try:
        for pos, q, kind, data, kw in sc.frames_iter():
            for m in (a, b):
                m.update(pos, q, kind, data, **kw)
        pa, ha = a.read_costmap()
        pb, hb = b.read_costmap()
        assert pa.tobytes() == pb.tobytes()
        for f in ("x_size", "y_size", "z_size", "x_origin", "y_origin", "z_origin", "width", "type"):
            assert getattr(ha, f) == getattr(hb, f)
        assert pb.dtype.itemsize == 8
    finally:
        a.close(); b.close()


def test_device_resident_readers_give_the_host_forms_bytes(oracle_lib):
    """VERDICT r4 'missing' #4 / 'next' #8: gie_query_global_dev (coordinates and records stay on the device, kernel on the mapper's
    stream — the integration the reference recommends for GPU planners, README.md:163-165), gie_read_costmap_dev, and the
    CostMap published through pinned memory on a copy stream (gie_costmap_publish / gie_costmap_acquire): byte for byte what the
    blocking host forms — which are held against the oracle — return, update after update; the payload handed out by one
    acquire survives the next publish (two pinned buffers alternate)."""
    import torch
    sc = parity.Scenario("dev_readers", (48, 40, 24), sensor="mixed", frames=4, delta_vox=5, yaw_deg=20.0)
    cfg = sc.config()
    a, b = OracleMapper(cfg), gie.Mapper(cfg)
    dev = torch.device("cuda", 0)
    X, Y, Z = sc.size
    try:
        stream = torch.cuda.ExternalStream(b.stream_handle(), device=dev)
        prev_view, prev_bytes = None, None
        for k, (pos, q, kind, data, kw) in enumerate(sc.frames_iter()):
            for m in (a, b):
                m.update(pos, q, kind, data, **kw)
            hdr_async = b.costmap_publish()               # enqueued behind the update; nobody waits
            pv = np.array(b.pivot())
            probes = (np.stack(np.meshgrid(np.arange(-9, X + 9, 3), np.arange(-9, Y + 9, 3), np.arange(-9, Z + 9, 3), indexing="ij"), -1).reshape(-1, 3) + pv).astype(np.int32)
            want_q = a.query_global(probes)
            assert np.array_equal(b.query_global(probes), want_q)
            with torch.cuda.stream(stream):
                d_xyz = torch.from_numpy(probes).to(dev)
                d_out = torch.zeros(probes.shape[0] * 20, dtype=torch.uint8, device=dev)
                b.query_global_dev(d_xyz.data_ptr(), probes.shape[0], d_out.data_ptr())
                d_cm = torch.zeros(X * Y * Z * 8, dtype=torch.uint8, device=dev)
                hdr_dev = b.read_costmap_dev(d_cm.data_ptr())
            stream.synchronize()
            assert d_out.cpu().numpy().tobytes() == want_q.tobytes()
            pa, ha = a.read_costmap()
            pb, hb = b.read_costmap()
            assert pa.tobytes() == pb.tobytes()
            assert d_cm.cpu().numpy().tobytes() == pb.tobytes()
            view = b.costmap_acquire(copy=False)
            assert view.tobytes() == pb.tobytes()
            for h in (hdr_async, hdr_dev):
                for f in ("x_size", "y_size", "z_size", "x_origin", "y_origin", "z_origin", "width", "type"):
                    assert getattr(h, f) == getattr(hb, f) == getattr(ha, f)
            if prev_view is not None:                      # the buffer of the publish before is still that update's
                assert prev_view.tobytes() == prev_bytes
            prev_view, prev_bytes = view, pb.tobytes()
    finally:
        a.close(); b.close()


def test_label_plane_read_in_place_or_copied_gives_the_same_map(oracle_lib):
    """gie_ogm_labels_dev_borrow may leave the plane where it is and let gie_fuse read it (round 5: `_inst_type` neither written nor
    reset) — unless something wants `_inst_type` first (gie_read_ogm, a second scan laid over it), which copies it after all; the
    plain gie_ogm_labels_dev copies, and its buffer may be overwritten right away.  Four HIP mappers fed the same device-resident
    planes — in place; read back in between; a point cloud on top; copied and overwritten — against the oracle fed the same way."""
    import torch
    from gie import scenes
    size = (64, 48, 40)                                   # X % 16 == 0: the in-place form applies
    cfg = gie.make_config(0.05, size, cutoff_dist=1.0)
    dev = torch.device("cuda", 0)
    ms = {k: gie.Mapper(cfg) for k in ("in_place", "read_back", "two_scans", "copied")}
    os_ = {k: OracleMapper(cfg) for k in ("plain", "two_scans")}
    rng = np.random.default_rng(3)
    try:
        for k in range(5):
            pos, q = scenes.pose(k, 0.05, delta_vox=5, yaw_deg=2.0)
            lab = np.ascontiguousarray(scenes.hash_world_labels(scenes.local_pivot(pos, 0.05, size), size, k, seed=9, p_occ=0.02).astype(np.int8))
            lab[rng.random(lab.shape) < 0.3] = 0            # a partly observed volume
            pts = (rng.uniform(-0.8, 0.8, size=(200, 3))).astype(np.float32)
            d_lab = torch.from_numpy(lab).to(dev)
            torch.cuda.synchronize()
            for name, m in ms.items():
                m.set_pose(pos, q)
                if name == "copied":
                    # the plain form copies: the caller's buffer may be overwritten as soon as the call's kernel has run
                    d_tmp = d_lab.clone()
                    torch.cuda.synchronize()
                    assert m.ogm_labels_dev(d_tmp.data_ptr()) is False
                    m.sync()
                    d_tmp.fill_(2)
                    torch.cuda.synchronize()
                else:
                    assert m.ogm_labels_dev(d_lab.data_ptr(), borrow=True) is True      # (X % 16 == 0, aligned, no robot sphere)
                if name == "read_back":
                    got = m.read_ogm()["inst_type"]
                    assert np.array_equal(got, lab)
                if name == "two_scans":
                    m.ogm_pointcloud(pts)
                m.step()
                m.sync()                                  # (d_lab is overwritten by the next frame's upload)
            for name, o in os_.items():
                o.set_pose(pos, q)
                o.ogm_labels(lab)
                if name == "two_scans":
                    o.ogm_pointcloud(pts)
                o.fuse(); o.batch_edt(); o.merge()
            for name, m in ms.items():
                want = os_["two_scans" if name == "two_scans" else "plain"].read_local()
                got = m.read_local()
                for key in ("type", "dist_sq", "coc"):
                    assert np.array_equal(want[key], got[key]), (k, name, key)
    finally:
        for m in list(ms.values()) + list(os_.values()):
            m.close()


def test_full_size_512_cube(oracle_lib):
    """BASELINE size: 512^3 @ 0.05 m (outside the reference's 11/11/10-bit envelope → wide mode).
    Two map updates against the oracle, every array bit for bit, plus size-independent
    properties of the result: every finite distance is witnessed by its closest obstacle, and
    a second update on an unchanged scene and pose changes nothing (idempotence)."""
    import bench
    from gie import scenes
    size = (512, 512, 512)
    cfg = gie.make_config(0.05, size, cutoff_dist=2.0, fast_mode=False)
    frames = bench.make_frames(scenes, 0.05, 2, 5, "vlp16_projective")
    rings, az, phi_min, phi_inc, bins = bench.SENSORS["vlp16_projective"]
    kw = dict(theta_inc=2.0 * np.pi / bins, theta_min=-np.pi, phi_inc=np.radians(phi_inc), phi_min=np.radians(phi_min))
    a, b = OracleMapper(cfg), gie.Mapper(cfg)
    try:
        for pos, q, img, _ in frames:
            for m in (a, b):
                m.update(pos, q, "multiscan", img, **kw)
            ea, eb = a.read_batch_edt(), b.read_batch_edt()
            assert np.array_equal(ea["dist_sq"], eb["dist_sq"]) and np.array_equal(ea["coc"], eb["coc"])
            del ea, eb
            ra, rb = a.read_local(), b.read_local()
            for key in ("type", "dist_sq", "coc"):
                assert np.array_equal(ra[key], rb[key]), key
            assert np.allclose(ra["edt"], rb["edt"], rtol=1e-6, atol=0)
            sa, sb = a.stats(), b.stats()
            for key in ("seeds_a", "seeds_b", "seeds_c", "visits_a", "visits_c", "levels_c", "blocks_total"):
                assert sa[key] == sb[key], key
        # witness property on the GPU result
        pv = np.array(b.pivot())
        known = (rb["type"] != 0) & (rb["dist_sq"] < 4000000)
        zz, yy, xx = np.nonzero(known)
        g = np.stack([xx, yy, zz], -1) + pv
        d = ((rb["coc"][known].astype(np.int64) - g) ** 2).sum(-1)
        assert np.array_equal(d, rb["dist_sq"][known])
        # idempotence: same pose, same frame again → same field
        pos, q, img, _ = frames[-1]
        b.update(pos, q, "multiscan", img, **kw)
        rc = b.read_local()
        assert np.array_equal(rc["dist_sq"][known], rb["dist_sq"][known])
    finally:
        a.close(); b.close()


def test_full_size_512_cube_hash_world(oracle_lib):
    """The bench's headline workload at full size (BASELINE config 5 on one 512^3 tile: hash world, full
    observation).  The scalar oracle is too slow for 134 M fully observed voxels, so the batch EDT is
    pinned by the INDEPENDENT multi-threaded CPU EDT (oracle/edt_mt.c, itself pinned by brute force):
    squared distances bit for bit, the closest obstacle as a witness.  After the merge: every voxel
    is known, its distance is witnessed by its closest obstacle, and never below the true distance."""
    from gie import scenes
    from oracle_py import edt_mt
    size = (512, 512, 512)
    cfg = gie.make_config(0.05, size, cutoff_dist=2.0, fast_mode=False)
    b = gie.Mapper(cfg)
    try:
        for k in range(2):
            pos, q = scenes.pose(k, 0.05, delta_vox=8, yaw_deg=2.0)
            lab = scenes.hash_world_labels(scenes.local_pivot(pos, 0.05, size), size, k, seed=5).astype(np.int8)
            b.set_pose(pos, q)
            b.ogm_labels(lab)
            b.fuse(); b.batch_edt()
            eb = b.read_batch_edt()
            ty = b.read_local(edt=False, dist_sq=False, coc=False)["type"]
            assert (ty != 0).all()
            d_cpu, _ = edt_mt(ty, want_coc=False)
            assert np.array_equal(eb["dist_sq"], d_cpu), "batch EDT differs in %d voxels" % int((eb["dist_sq"] != d_cpu).sum())
            c = eb["coc"]
            assert (ty[c[..., 2], c[..., 1], c[..., 0]] == 2).all()
            zz, yy, xx = np.meshgrid(np.arange(512, dtype=np.int32), np.arange(512, dtype=np.int32), np.arange(512, dtype=np.int32), indexing="ij")
            assert np.array_equal((xx - c[..., 0]) ** 2 + (yy - c[..., 1]) ** 2 + (zz - c[..., 2]) ** 2, d_cpu)
            del eb, c, xx, yy, zz
            b.merge()
            rb = b.read_local(edt=False)
            st = b.stats()
            pv = np.array(b.pivot(), dtype=np.int64)
            # d_cpu only knows the obstacles INSIDE the volume.  A closest obstacle inside the volume can never be
            # closer than that; one outside it (an obstacle the volume has left behind: limited observation, waves)
            # may be, and then it has to be a voxel the global map believes occupied
            cl = rb["coc"].astype(np.int64) - pv
            inside = ((cl >= 0) & (cl < 512)).all(-1)
            assert (rb["dist_sq"][inside] >= d_cpu[inside]).all()
            assert (rb["dist_sq"][~inside] <= d_cpu[~inside]).all()
            if k == 0:
                assert inside.all() and np.array_equal(rb["dist_sq"], d_cpu)     # nothing is known outside yet
            else:
                assert 0 < int((~inside).sum()) < 0.05 * inside.size
                far = np.ascontiguousarray(rb["coc"][~inside][::97][:4096], dtype=np.int32)
                assert (b.query_global(far)["vox_type"] == 2).all()
            assert float((rb["dist_sq"][inside] == d_cpu[inside]).mean()) > 0.999
            g = np.stack(np.meshgrid(np.arange(512), np.arange(512), np.arange(512), indexing="ij")[::-1], -1) + pv
            assert np.array_equal(((rb["coc"].astype(np.int64) - g) ** 2).sum(-1), rb["dist_sq"])
            if k == 1:
                assert st["visits_a"] + st["visits_b"] + st["visits_c"] > 0
            del rb, g, d_cpu, ty, cl, inside
    finally:
        b.close()


@pytest.mark.gpu
def test_full_size_512_cube_flood_of_wave_c(oracle_lib):
    """A FLOOD at full size (BASELINE config 3's regime: 512^3, 16-ring lidar through the projective OGM, waves A / B / C): the
    bench's `vlp16_projective` workload until an update in which a box of the world has vanished and wave C re-floods what it
    shadowed — millions of visits, dozens of tile rounds (frame 7: 10 M visits in 50 rounds).  The scalar oracle needs minutes per
    update at this size, so the result is pinned by what it has to be: every known voxel's distance is witnessed by its closest
    obstacle; a closest obstacle inside the volume is an OCCUPIED voxel and exactly as far as the independent exact CPU EDT of
    the volume's own obstacles says (oracle/edt_mt.c, pinned by brute force); one outside the volume is at most that far and
    a voxel the global map believes occupied."""
    import bench
    from gie import scenes
    from oracle_py import edt_mt
    size = (512, 512, 512)
    cfg = gie.make_config(0.05, size, cutoff_dist=2.0, fast_mode=False)
    rings, az, phi_min, phi_inc, bins = bench.LIDARS["vlp16_projective"]
    kw = dict(theta_inc=2.0 * np.pi / bins, theta_min=-np.pi, phi_inc=np.radians(phi_inc), phi_min=np.radians(phi_min))
    world = bench.lidar_world(scenes)
    b = gie.Mapper(cfg)
    try:
        flooded = False
        for k in range(12):
            pos, q, img, _ = bench.lidar_host_frame(scenes, world, 0.05, "vlp16_projective", k)
            b.set_pose(pos, q)
            b.ogm_multiscan(img, **kw)
            b.step()
            st = b.stats()
            if st["visits_c"] < 1000000:
                continue
            flooded = True
            assert st["levels_c"] >= 10
            rb = b.read_local(edt=False)
            ty = rb["type"]
            known = (ty != 0) & (rb["dist_sq"] < 4000000)
            d_cpu, _ = edt_mt(ty, want_coc=False)
            pv = np.array(b.pivot(), dtype=np.int64)
            cl = rb["coc"].astype(np.int64) - pv
            inside = ((cl >= 0) & (cl < 512)).all(-1) & known
            outside = known & ~inside
            assert int(known.sum()) > 20000000 and inside.any() and outside.any()
            assert np.array_equal(rb["dist_sq"][inside], d_cpu[inside]), "%d voxels differ from the exact EDT" % int((rb["dist_sq"][inside] != d_cpu[inside]).sum())
            ci = cl[inside]
            assert (ty[ci[:, 2], ci[:, 1], ci[:, 0]] == 2).all()
            assert (rb["dist_sq"][outside] <= d_cpu[outside]).all()
            far = np.ascontiguousarray(rb["coc"][outside][::997][:4096], dtype=np.int32)
            assert (b.query_global(far)["vox_type"] == 2).all()
            zz, yy, xx = np.nonzero(known)
            g = np.stack([xx, yy, zz], -1) + pv
            assert np.array_equal(((rb["coc"][known].astype(np.int64) - g) ** 2).sum(-1), rb["dist_sq"][known])
            break
        assert flooded, "no flood within 12 updates"
    finally:
        b.close()


@pytest.mark.gpu
def test_full_size_512_cube_ray_casting(oracle_lib):
    """The bench's default workload at full size: 512^3 @ 0.05 m, VLP-16 cloud through parallel
    ray casting (sparse observation: tile lists, direct pass Z, scan labels on demand).  Three map
    updates against the oracle, every array bit for bit, and the scan (labels + counts) of the
    last one."""
    import bench
    from gie import scenes
    size = (512, 512, 512)
    cfg = gie.make_config(0.05, size, cutoff_dist=2.0, fast_mode=False)
    frames = bench.make_frames(scenes, 0.05, 3, 5, "vlp16")
    a, b = OracleMapper(cfg), gie.Mapper(cfg)
    try:
        for k, (pos, q, pts, _) in enumerate(frames):
            for m in (a, b):
                m.set_pose(pos, q)
                m.ogm_pointcloud(pts)
            if k == len(frames) - 1:
                oa, ob = a.read_ogm(), b.read_ogm()
                assert np.array_equal(oa["ray_count"], ob["ray_count"]) and np.array_equal(oa["inst_type"], ob["inst_type"])
                del oa, ob
            for m in (a, b):
                m.fuse(); m.batch_edt(); m.merge()
            ra, rb = a.read_local(), b.read_local()
            for key in ("type", "dist_sq", "coc"):
                assert np.array_equal(ra[key], rb[key]), (k, key)
            assert np.allclose(ra["edt"], rb["edt"], rtol=1e-6, atol=0)
            sa, sb = a.stats(), b.stats()
            for key in ("seeds_a", "seeds_b", "seeds_c", "visits_a", "visits_c", "levels_c", "blocks_total"):
                assert sa[key] == sb[key], (k, key)
            del ra, rb
    finally:
        a.close(); b.close()


@pytest.mark.gpu
def test_full_size_512_cube_c5_headline(oracle_lib):
    """The bench's headline workload ITSELF at full size: BASELINE config 5's hash world on one 512^3 tile @ 0.05 m, every voxel
    observed, a quarter of the obstacles toggling, the robot moving 8 voxels per update — six map updates against the oracle,
    every array bit for bit and every wave statistic (waves A / B / C visit 24 k / 36 k / 20 k voxels per update here; the small
    scenarios above have a few hundred).  tools/soak_fullsize.py --c5 is the longer form (profiles/r03_soak_fullsize_c5_6_updates.log).
    Round 6: the GLOBAL map is compared after every update too — 20 000 probes in and around the volume and 6 000
    in the slabs the robot has just left — because at this size 82 % of the tiles are `tskip` tiles whose stored records live in
    the pair plane ("deferred records"): update 2 is the first that defers, update 3 jumps sideways (tiles lose flag 2 in bulk:
    k_coc_catchup_new with 64 z-tiles per column), update 4 runs with the changed-block flags on (the reference's order of kernels:
    gie_catchup_everything at 512^3 — unify_helper.cuh:448-523 stores every observed voxel every frame), update 5 is fused again."""
    import bench
    from gie import scenes
    size = (512, 512, 512)
    cfg = gie.make_config(0.05, size, cutoff_dist=2.0, fast_mode=False)
    a, b = OracleMapper(cfg), gie.Mapper(cfg)
    rng = np.random.default_rng(2026)
    extra = {3: (19, -13, 6), 4: (19, -13, 6), 5: (19, -13, 6)}       # voxels on top of the drive from update 3 on: a jump off the block grid
    prev_pvt = None
    try:
        for k in range(6):
            pos, q = bench.c5_pose(scenes, k, 0.05)
            pos = tuple(np.float32(float(pos[i]) + extra.get(k, (0, 0, 0))[i] * 0.05) for i in range(3))
            lab = np.ascontiguousarray(scenes.hash_world_labels(scenes.local_pivot(pos, 0.05, size), size, k, seed=bench.C5["seed"],
                                                                p_occ=bench.C5["p_occ"], toggle_frac=bench.C5["toggle_frac"]).astype(np.int8))
            for m in (a, b):
                m.stream_enable(k == 4)
                m.update(pos, q, "labels", lab)
            if k == 4:
                assert a.stream_count() == b.stream_count() > 250000      # (blocks flagged as changed; not drained: 2.9 GB per mapper)
            ra, rb = a.read_local(), b.read_local()
            for key in ("type", "dist_sq", "coc"):
                assert np.array_equal(ra[key], rb[key]), (k, key)
            assert np.allclose(ra["edt"], rb["edt"], rtol=1e-6, atol=0)
            sa, sb = a.stats(), b.stats()
            for key in ("seeds_a", "seeds_b", "seeds_c", "visits_a", "visits_b", "visits_c", "levels_a", "levels_b", "levels_c", "blocks_total"):
                assert sa[key] == sb[key], (k, key, sa[key], sb[key])
            if k > 0:
                assert sb["visits_a"] > 10000 and sb["visits_b"] > 10000 and sb["visits_c"] > 10000
            del ra, rb, lab
            assert a.pivot() == b.pivot()
            parity.compare_global("update %d, in and around the volume" % k, a, b, parity.probe_coords(a.pivot(), size, rng, n=20000, margin=12))
            if prev_pvt is not None:
                gone = parity.probe_left_behind(prev_pvt, a.pivot(), size, rng)
                assert len(gone) > 1000
                parity.compare_global("update %d, the slabs just left" % k, a, b, gone)
            prev_pvt = a.pivot()
    finally:
        a.close(); b.close()


@pytest.mark.gpu
def test_partial_pass_z_covers_every_reader(oracle_lib, monkeypatch):
    """The map update only produces the batch EDT where Mark reads it (tiles with a known voxel; wave B
    computes the distance of an unknown face voxel on demand).  Exported without completion, it
    must equal the oracle on exactly those tiles; the completed export equals it everywhere
    (checked by every other parity test)."""
    sc = parity.Scenario("partial_z", (96, 80, 72), sensor="lidar_points", frames=3, lidar_az=360, extent=(4.0, 3.5, 3.0))
    cfg = sc.config()
    from hooks_py import HooksMapper
    monkeypatch.setenv("GIE_EDT_EXPORT_PARTIAL", "1")
    a, b = OracleMapper(cfg), HooksMapper(cfg)
    try:
        for pos, q, kind, data, kw in sc.frames_iter():
            for m in (a, b):
                m.set_pose(pos, q); m.ogm_pointcloud(data); m.fuse(); m.batch_edt()
            ea, eb = a.read_batch_edt(), b.read_batch_edt()
            ty = a.read_local(edt=False, dist_sq=False, coc=False)["type"]
            Z, Y, X = ty.shape
            kn = np.zeros(((Z + 7) // 8, (Y + 7) // 8, (X + 7) // 8), bool)
            zz, yy, xx = np.nonzero(ty != 0)
            kn[zz // 8, yy // 8, xx // 8] = True
            need = np.repeat(np.repeat(np.repeat(kn, 8, 0), 8, 1), 8, 2)[:Z, :Y, :X]
            assert 0.01 < need.mean() < 0.9
            assert np.array_equal(ea["dist_sq"][need], eb["dist_sq"][need])
            assert np.array_equal(ea["coc"][need], eb["coc"][need])
            for m in (a, b):
                m.merge()
            ra, rb = a.read_local(), b.read_local()
            for key in ("type", "dist_sq", "coc"):
                assert np.array_equal(ra[key], rb[key]), key
    finally:
        a.close(); b.close()


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["0", "1"])
def test_tile_list_and_sweep_modes_agree_with_the_oracle(oracle_lib, monkeypatch, mode):
    """Mark, obtainFrontiers, commit and pass Z either sweep the volume or walk the lists of tiles
    that hold something (chosen by each kernel from the length of its list).  Both forms must
    be bit-exact; GIE_TILE_LIST forces one.  The library reads the variable once per process, so
    each mode runs in its own interpreter."""
    import subprocess, sys, os
    code = (
        "import sys; sys.path[:0] = [%r, %r, %r]\n"
        "import gie, parity\n"
        "from oracle_py import OracleMapper\n"
        "for sensor, fast in (('mixed', False), ('lidar_points', False), ('depth', True)):\n"
        "    sc = parity.Scenario('modes_' + sensor, (72, 64, 40), sensor=sensor, frames=5, fast_mode=fast, lidar_az=360)\n"
        "    parity.run_and_compare(sc, OracleMapper, gie.Mapper)\n"
        "print('ok')\n"
    ) % (os.path.join(parity.__file__.rsplit('/', 2)[0]), os.path.join(parity.__file__.rsplit('/', 2)[0], 'gie-mapping_amd'),
         os.path.dirname(parity.__file__))
    import hooks_py
    hooks_py.load()                                   # (builds the test library if need be, outside the child)
    env = dict(os.environ, GIE_TILE_LIST=mode, GIE_LIB=hooks_py.TEST_SO)       # the package loads the test build: the product library has no switches
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True)
    assert r.returncode == 0 and "ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


@pytest.mark.gpu
def test_long_run_robot_travels_and_returns(oracle_lib):
    """Sixty map updates with the robot travelling three volume widths away and back through a
    changing scene: blocks leave the local volume and come back, tile flags / stamps / lists are
    reused frame after frame.  Every array bit for bit every frame (parity.run_and_compare)."""
    sc = parity.Scenario("long_run", (64, 56, 32), sensor="mixed", frames=60, delta_vox=7, yaw_deg=23.0, n_boxes=80,
                         extent=(10.0, 5.0, 1.5), toggle=0.3)
    # there and back again: scenes.pose(k) moves along +x; mirror the second half
    orig = sc.frames_iter
    def there_and_back():
        fr = list(orig())
        half = len(fr) // 2
        for k, f in enumerate(fr):
            yield f if k < half else (fr[len(fr) - 1 - k][0], fr[len(fr) - 1 - k][1]) + f[2:]
    sc.frames_iter = there_and_back
    out = parity.run_and_compare(sc, OracleMapper, gie.Mapper)
    assert len(out) == 60
    assert sum(s["visits_c"] for s in out) > 0 and max(s["blocks_total"] for s in out) > 300


@pytest.mark.gpu
def test_block_pool_overflow_fails_loudly():
    """A pool that is too small is a sticky, reported error (never a silent wrong map or a crash)."""
    sc = parity.Scenario("tiny_pool", (64, 64, 32), sensor="depth", frames=3)
    cfg = gie.make_config(sc.voxel, sc.size, cutoff_dist=1.0, max_blocks=7)
    m = gie.Mapper(cfg)
    with pytest.raises(RuntimeError) as e:
        for pos, q, kind, data, kw in sc.frames_iter():
            m.update(pos, q, kind, data, **kw)
            m.sync()
    assert "block pool" in str(e.value)
    m.close()


@pytest.mark.gpu
def test_edge_inputs(oracle_lib):
    """Empty scans, NaN / Inf / far / duplicate / zero-length points, negative far-away poses,
    images without a valid reading (tests/edge_inputs.py): HIP equals the oracle on all of them."""
    import edge_inputs
    edge_inputs.run(OracleMapper, gie.Mapper)


@pytest.mark.parametrize("sc", [s for s in SCENARIOS if s.name in ("raycast", "mixed", "fast_mode", "planner_boxes", "c3_no_cutoff",
                                                                  "c5_hash_world", "thin_x", "odd_dims")], ids=lambda s: s.name)
def test_hip_matches_oracle_production_sequence(oracle_lib, sc):
    """set_pose / ogm / step() only: unlabelled ray-cast scans, partial or direct pass Z, Mark + commit fused —
    exactly what a node runs (the stage-by-stage tests call readers in between that complete those stages)."""
    parity.run_and_compare(sc, OracleMapper, gie.Mapper, production=True)


@pytest.mark.gpu
@pytest.mark.parametrize("wgs", ["8", "24"])
@pytest.mark.parametrize("name", ["c5_hash_world", "mixed", "c3_no_cutoff"])
def test_small_wavefront_grids(oracle_lib, monkeypatch, name, wgs):
    """gie_config.wave_workgroups shrinks the persistent grid of the wavefront kernel (processes that share a device):
    levels and tile rounds are split over fewer workgroups, the tails of waves A / B reach workgroup 0 at other levels — same results."""
    sc = [s for s in SCENARIOS if s.name == name][0]

    def small_grid(cfg):
        c = type(cfg).from_buffer_copy(cfg)
        c.wave_workgroups = int(wgs)
        return gie.Mapper(c)
    parity.run_and_compare(sc, OracleMapper, small_grid, production=True)


@pytest.mark.gpu
def test_waves_wait_out_a_kernel_that_holds_every_compute_unit(oracle_lib):
    """The wavefront kernel meets at a hand-rolled grid barrier, so all of its workgroups have to be resident at
    once.  Here another stream fills EVERY wave slot of the device with spinning workgroups (tests/gpu_helpers)
    for a quarter of a second per map update, launched right before the update: the map update — wave A, B
    and C seeded, several barrier rounds each — has to sit the intruder out and still equal the oracle bit for
    bit, without a barrier timeout."""
    import ctypes as C
    import os
    so = os.path.join(os.path.dirname(os.path.abspath(__file__)), "gpu_helpers", "libspin.so")
    if not os.path.exists(so):
        pytest.skip("tests/gpu_helpers/libspin.so not built (__graft_entry__.build())")
    gie.load_library()                                                   # first: one HIP runtime per process (gie/mapper.py load_library) — the helper must bind to the one the mapper uses
    spin = C.CDLL(so)
    spin.spin_start.argtypes = [C.c_int, C.c_double]
    sc = parity.Scenario("vlp16", (48, 48, 16), sensor="multiscan", frames=10, delta_vox=5, yaw_deg=10.0)
    cfg = sc.config()
    a, b = OracleMapper(cfg), gie.Mapper(cfg)
    try:
        visits = 0
        for k, (pos, q, kind, data, kw) in enumerate(sc.frames_iter()):
            for m in (a, b):
                m.set_pose(pos, q)
                parity._feed(m, kind, data, kw)
            a.step()
            assert spin.spin_start(2 if k % 2 else 1, 250.0) == 0      # 2 x 1024 threads per CU = every wave slot; 1 = half of them
            b.step()                                                    # enqueued while the intruder is resident
            b.sync()                                                    # raises on GIE_ERR_TIMEOUT
            assert spin.spin_wait() == 0
            ra, rb = a.read_local(), b.read_local()
            for key in ("type", "dist_sq", "coc"):
                assert np.array_equal(ra[key], rb[key]), (k, key)
            sa, sb = a.stats(), b.stats()
            for key in ("visits_a", "visits_c", "levels_a", "levels_b", "levels_c"):
                assert sa[key] == sb[key], (k, key)
            visits += sa["visits_a"] + sa["visits_b"] + sa["visits_c"]
        assert visits > 0
    finally:
        a.close(); b.close()


IRREGULAR = [("mixed", (3, 6), ()), ("blink_empty_scans", (3, 6, 7, 11), ()), ("c5_hash_world", (2, 3, 5), ()), ("retain_odd_r1", (2, 5, 6), ()),
             ("mixed", (), (3, 4, 8)), ("blink_empty_scans", (5, 12), (3, 4, 9, 10, 13)), ("c5_128cube", (1, 3), ())]


@pytest.mark.gpu
@pytest.mark.parametrize("fuse_only,stream_on", [((3,), ()), ((3,), (5,)), ((2, 3), ())], ids=["f3", "f3-s5", "f2_3"])
def test_fuse_without_merge_then_jump(oracle_lib, fuse_only, stream_on):
    """parity.FUSE_ONLY_THEN_JUMP: an abandoned fuse's tiles flagged 1 hold deferred records too (round 6)."""
    parity.run_irregular(parity.FUSE_ONLY_THEN_JUMP, OracleMapper, gie.Mapper, fuse_only=set(fuse_only), stream_on=set(stream_on))


@pytest.mark.gpu
@pytest.mark.parametrize("name,fuse_only,stream_on", IRREGULAR, ids=["%s-f%s-s%s" % (n, "_".join(map(str, f)), "_".join(map(str, s))) for n, f, s in IRREGULAR])
def test_irregular_call_orders(oracle_lib, name, fuse_only, stream_on):
    """gie_fuse without a merge behind it, and runs that change between the fused sweep and the reference's order (see
    tests/test_host_logic.py::test_irregular_call_orders_emulation)."""
    sc = [s for s in SCENARIOS if s.name == name][0]
    parity.run_irregular(sc, OracleMapper, gie.Mapper, fuse_only=set(fuse_only), stream_on=set(stream_on))


@pytest.mark.gpu
def test_jumping_robot_keeps_the_hash_table_alive(oracle_lib):
    from test_host_logic import _jumping_robot
    _jumping_robot(gie.Mapper, updates=300)


@pytest.mark.gpu
@pytest.mark.parametrize("stream", [False, True], ids=["fused", "changed_block_flags"])
def test_barrier_timeout_leaves_what_gie_h_says(oracle_lib, stream):
    """GIE_ERR_TIMEOUT (include/gie.h:28-35), forced: `gie_debug_fault_barrier` makes the wavefront launch of one map update
    meet at a barrier that waits for a workgroup that does not exist (short spin limit), the path a second process
    holding the compute units would take.  What the header promises, checked on a drive with seeds of all three
    waves: the condition is reported once; Mark's own distances are committed when Mark and commit are one sweep
    (the state of the oracle after Mark + UpdateHashBatch without the waves: go_merge_begin_tiled), nothing of the
    update is committed when the changed-block flags are on (the stored records of the voxels known before are the
    ones from before the update); the next updates run normally — no error, waves with visits again."""
    import ctypes as C
    sc = parity.Scenario("c3_no_cutoff", (56, 56, 20), voxel=0.1, sensor="multiscan", frames=10, delta_vox=6, yaw_deg=12.0,
                         cutoff_dist=100.0, extent=(5.0, 5.0, 1.5))
    cfg = sc.config()
    from hooks_py import HooksMapper                   # gie_debug_fault_barrier exists in the test build of the library only
    a, b = OracleMapper(cfg), HooksMapper(cfg)
    fault = lambda h, n: b.debug_fault_barrier(n)      # noqa: E731
    try:
        if stream:
            a.stream_enable(True); b.stream_enable(True)
        faulted = -1
        visits_after = 0
        for k, (pos, q, kind, data, kw) in enumerate(sc.frames_iter()):
            for m in (a, b):
                m.set_pose(pos, q)
                parity._feed(m, kind, data, kw)
            if faulted < 0 and k >= 6:                     # (frame 6 of this drive seeds all three waves: 141 / 226 / 40)
                # the oracle one stage at a time: does this update seed the waves?  (decided after Mark: look at a copy's statistics)
                a.fuse(); a.batch_edt()
                X, Y, Z = sc.size
                pv = np.array(a.pivot())
                zz, yy, xx = np.meshgrid(np.arange(Z), np.arange(Y), np.arange(X), indexing="ij")
                xyz = (np.stack([xx, yy, zz], -1).reshape(-1, 3) + pv).astype(np.int32)
                before = b.query_global(xyz)
                a.merge_begin_tiled()                      # Mark + UpdateHashBatch, no obtainFrontiers, no waves
                assert fault(b._h, 1) == 0
                b.step()
                with pytest.raises(RuntimeError, match=r"\(4\)"):      # GIE_ERR_TIMEOUT
                    b.sync()
                b.sync()                                   # reported once
                sb = b.stats()
                assert sb["seeds_a"] + sb["seeds_b"] + sb["seeds_c"] > 0, "the faulted update has to have seeds (choose another frame)"
                after = b.query_global(xyz)
                known_before = before["vox_type"] != 0
                if stream:
                    for key in ("dist_sq", "coc"):
                        assert np.array_equal(before[key][known_before], after[key][known_before]), key
                else:
                    ra, rb = a.read_local(edt=False), b.read_local(edt=False)
                    known = ra["type"] != 0
                    assert np.array_equal(ra["type"] != 0, rb["type"] != 0)
                    for key in ("dist_sq", "coc"):
                        assert np.array_equal(ra[key][known], rb[key][known]), "local " + key
                    ga = a.query_global(xyz)
                    kn = ga["vox_type"] != 0
                    for key in ("dist_sq", "coc"):
                        assert np.array_equal(ga[key][kn], after[key][kn]), "stored " + key
                faulted = k
                a.merge_end()                              # (the oracle goes on as if nothing had happened: only the types are compared below)
                continue
            a.step()
            b.step()
            b.sync()                                       # no error left over
            ta, tb = a.read_local(edt=False, dist_sq=False, coc=False)["type"], b.read_local(edt=False, dist_sq=False, coc=False)["type"]
            assert np.array_equal(ta != 0, tb != 0), k     # (known / unknown does not depend on the waves)
            if faulted >= 0:
                s = b.stats()
                visits_after += s["visits_a"] + s["visits_b"] + s["visits_c"]
        assert faulted >= 0 and visits_after > 0
    finally:
        a.close()
        b.close()
