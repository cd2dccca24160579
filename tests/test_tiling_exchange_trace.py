"""The call sequences of the eight exchange functions of gie/tiling.py, held against recorded traces.

What a round does on the device is the business of test_tiling_halo.py and test_multi_rank_gloo.py.  This test holds the
PROTOCOL: which Mapper calls every tile receives and which torch.distributed calls every rank makes, in which order and with
which arguments — per-face or all-faces calls, the sorted face order, where sync() and torch.cuda.synchronize fall, sparse
count batches before data batches, empty sends / receives left out, the copy + all-reduce(max) behind every gated round.
Mappers, transport and the few torch calls involved are fakes that log; nothing runs on a device.

test_tiling_exchange_trace.json holds the traces of the six forms that run with device "cpu" since before they shared one round
loop: `record_all` of this module, run against that earlier tiling.py (call names and small integers only, one scenario per
line).  After a deliberate change of the protocol, dump record_all(tiling, torch_log) over it and say in the change what moved.
The two fixed-rounds forms are held against their gated siblings: the same trace without the gate."""
import ctypes
import itertools
import json
import os

import numpy as np
import pytest
import torch

from gie import tiling
from gie.mapper import HALO_DTYPE, HALO_ENTRY_DTYPE

TRACES = os.path.join(os.path.dirname(os.path.abspath(__file__)), "test_tiling_exchange_trace.json")
FACE = 16                                   # tiles of 4x4x4: every face layer holds 16 voxels
GRIDS = [(2, 1, 1), (2, 2, 1)]              # one shared face; two faces per tile, so the sorted face order matters
SCRIPTS = {"stable": ([3, 0], 2), "bound": ([1], 3)}   # what refine() returns, cycled -> the rounds an until-stable form runs (max_rounds=3)
CALLS = 2                                   # every scenario runs twice on the same `bufs`: the second call must reuse what the first built


def _known(tile, face):
    """Entries of a sparse layer: none on faces 0 / 1 of tile 0, so that an empty send has to be left out."""
    return 3 * tile + 2 * (face // 2)


class Log(list):
    """(who, call, arguments); device pointers become 0, 1, 2, ... by order of first appearance."""

    def __init__(self):
        super().__init__()
        self.ptrs = {}

    def ptr(self, p):
        return None if p is None else self.ptrs.setdefault(int(p), len(self.ptrs))

    def add(self, who, call, *args):
        self.append([who, call, list(args)])


class FakeMapper:
    def __init__(self, tile, log, script):
        self.tile, self.log, self.seeds = tile, log, itertools.cycle(script)

    def _ptrs(self, dptrs):
        return [[f, self.log.ptr(p)] for f, p in sorted(dptrs.items())]

    def halo_count(self, face):
        self.log.add(self.tile, "halo_count", face)
        return FACE

    def halo_export(self, face):
        self.log.add(self.tile, "halo_export", face)
        return np.zeros(FACE, HALO_DTYPE)

    def halo_import(self, face, layer):
        self.log.add(self.tile, "halo_import", face, str(layer.dtype == HALO_DTYPE), len(layer))

    def halo_export_sparse(self, face):
        self.log.add(self.tile, "halo_export_sparse", face)
        return np.zeros(_known(self.tile, face), HALO_ENTRY_DTYPE)

    def halo_import_sparse(self, face, entries):
        self.log.add(self.tile, "halo_import_sparse", face, str(entries.dtype == HALO_ENTRY_DTYPE), len(entries))

    def halo_export_dev(self, face, dptr):
        self.log.add(self.tile, "halo_export_dev", face, self.log.ptr(dptr))

    def halo_import_dev(self, face, dptr):
        self.log.add(self.tile, "halo_import_dev", face, self.log.ptr(dptr))

    def halo_export_sparse_dev(self, face, dptr, dcount):
        self.log.add(self.tile, "halo_export_sparse_dev", face, self.log.ptr(dptr), self.log.ptr(dcount))
        ctypes.c_int32.from_address(dcount).value = _known(self.tile, face)      # device "cpu": the count word is host memory

    def halo_import_sparse_dev(self, face, dptr, dcount):
        self.log.add(self.tile, "halo_import_sparse_dev", face, self.log.ptr(dptr), self.log.ptr(dcount), ctypes.c_int32.from_address(dcount).value)

    def halo_export_all_dev(self, dptrs):
        self.log.add(self.tile, "halo_export_all_dev", self._ptrs(dptrs))

    def halo_import_all_dev(self, dptrs):
        self.log.add(self.tile, "halo_import_all_dev", self._ptrs(dptrs))

    def merge_end(self):
        self.log.add(self.tile, "merge_end")

    def refine(self):
        n = next(self.seeds)
        self.log.add(self.tile, "refine", n)
        return n

    def refine_async(self):
        self.log.add(self.tile, "refine_async")

    def refine_dev(self, d_changed):
        self.log.add(self.tile, "refine_dev", self.log.ptr(d_changed))

    def round_gate(self, d_go):
        self.log.add(self.tile, "round_gate", self.log.ptr(d_go))

    def round_end(self, d_go):
        self.log.add(self.tile, "round_end", self.log.ptr(d_go))

    def sync(self):
        self.log.add(self.tile, "sync")

    def stream_handle(self):
        self.log.add(self.tile, "stream_handle")
        return 0


class _Work:
    def wait(self):
        pass


class FakeDist:
    """torch.distributed as one rank sees it.  Logs kind, peer and element count of every op of a batch, and every reduce; moves
    no data: a reduce leaves its tensor alone (the rank's own seed count decides), and a one-element receive — the entry count of a
    sparse layer — is set to peer + 1 so that the data receive behind it has a length."""
    isend, irecv = "isend", "irecv"

    class ReduceOp:
        SUM, MAX = "sum", "max"

    class P2POp:
        def __init__(self, op, tensor, peer, group=None):
            self.op, self.tensor, self.peer, self.group = op, tensor, peer, group

    def __init__(self, rank, log):
        self.who, self.log = "rank%d" % rank, log

    def batch_isend_irecv(self, ops):
        self.log.add(self.who, "batch_isend_irecv", [[o.op, o.peer, o.tensor.numel(), o.group] for o in ops])
        for o in ops:
            if o.op == self.irecv and o.tensor.numel() == 1:
                o.tensor.fill_(o.peer + 1)
        return [_Work() for _ in ops]

    def all_reduce(self, t, op=None, group=None):
        self.log.add(self.who, "all_reduce", op, t.numel(), int(t.flatten()[0].item()), group)


@pytest.fixture
def torch_log(monkeypatch):
    """The torch calls that belong to the protocol, logged into whatever log is current: torch.cuda.synchronize (logged only),
    Tensor.copy_ and torch.amax (logged, then done)."""
    cur = {"log": None}
    copy_, amax = torch.Tensor.copy_, torch.amax

    def log_copy(self, src, *a, **kw):
        cur["log"].add("torch", "copy_", self.numel(), src.numel())
        return copy_(self, src, *a, **kw)

    def log_amax(t, *a, **kw):
        cur["log"].add("torch", "amax", t.numel(), kw["out"].numel())
        return amax(t, *a, **kw)

    monkeypatch.setattr(torch.cuda, "synchronize", lambda device=None: cur["log"].add("torch", "cuda.synchronize", str(device)))
    monkeypatch.setattr(torch.Tensor, "copy_", log_copy)
    monkeypatch.setattr(torch, "amax", log_amax)
    return cur


def _trace_local(cur, fn, grid, script, *args, **kw):
    """[return value of the last call, log] of an in-process form: fn(mappers, grid, *args, **kw), CALLS times."""
    log = cur["log"] = Log()
    ms = [FakeMapper(r, log, script) for r in range(grid[0] * grid[1] * grid[2])]
    for c in range(CALLS):
        log.add("test", "call", c)
        ret = fn(ms, grid, *args, **kw)
    return [ret, list(log)]


def _trace_ranked(cur, fn, grid, script, make_args):
    """{rank: [return value, log]} of a ranked form, one rank after the other: fn(mapper, dist, rank, world, *args, **kw) with
    (args, kw) = make_args() made afresh for every rank (its `bufs`)."""
    world, out = grid[0] * grid[1] * grid[2], {}
    for rank in range(world):
        log = cur["log"] = Log()
        m, dist = FakeMapper(rank, log, script), FakeDist(rank, log)
        args, kw = make_args()
        for c in range(CALLS):
            log.add("test", "call", c)
            ret = fn(m, dist, rank, world, *args, **kw)
        out["rank%d" % rank] = [ret, list(log)]
    return out


def _grid_name(grid):
    return "x".join(str(g) for g in grid)


CPU = torch.device("cpu")
BOUNDS = [1, 3]


def record_all(t, cur):
    """{scenario: trace} of the six forms of tiling module `t` that run with device "cpu" whether or not they share code."""
    out = {}
    for grid in GRIDS:
        g = _grid_name(grid)
        for name, (script, _) in SCRIPTS.items():
            for sparse in (False, True):
                s = "%s|%s|%s" % (g, name, "sparse" if sparse else "dense")
                out["exchange_until_stable_local|" + s] = _trace_local(cur, t.exchange_until_stable_local, grid, script, max_rounds=3, sparse=sparse, sent=[])
                out["exchange_until_stable|" + s] = _trace_ranked(cur, t.exchange_until_stable, grid, script, lambda: ((), dict(max_rounds=3, group="g", sparse=sparse)))
                out["exchange_until_stable_device|" + s] = _trace_ranked(cur, t.exchange_until_stable_device, grid, script,
                                                                        lambda: ((CPU,), dict(bufs={}, max_rounds=3, group="g", sparse=sparse)))
            out["exchange_until_stable_local_device|%s|%s" % (g, name)] = _trace_local(cur, t.exchange_until_stable_local_device, grid, script, CPU, max_rounds=3, bufs={})
        for n in BOUNDS:
            out["exchange_converged_local_device|%s|%d" % (g, n)] = _trace_local(cur, t.exchange_converged_local_device, grid, [0], CPU, max_rounds=n, bufs={})
            out["exchange_converged_device|%s|%d" % (g, n)] = _trace_ranked(cur, t.exchange_converged_device, grid, [0], lambda: ((CPU, {}), dict(max_rounds=n, group="g")))
    return out


def test_traces_equal_the_recorded_ones(torch_log):
    """Entry for entry, return values included (json round trip: tuples and lists compare equal)."""
    with open(TRACES) as f:
        want = json.load(f)
    got = json.loads(json.dumps(record_all(tiling, torch_log)))
    assert sorted(got) == sorted(want)
    for key in sorted(want):
        assert got[key] == want[key], key


@pytest.mark.parametrize("grid", GRIDS, ids=_grid_name)
@pytest.mark.parametrize("name", sorted(SCRIPTS))
def test_until_stable_returns_the_rounds_run(torch_log, grid, name):
    script, rounds = SCRIPTS[name]
    for sparse in (False, True):
        assert _trace_local(torch_log, tiling.exchange_until_stable_local, grid, script, max_rounds=3, sparse=sparse)[0] == rounds
        for fn, args in ((tiling.exchange_until_stable, ()), (tiling.exchange_until_stable_device, (CPU,))):
            got = _trace_ranked(torch_log, fn, grid, script, lambda: (args, dict(max_rounds=3, sparse=sparse)))
            assert [ret for ret, _ in got.values()] == [rounds] * len(got)
    assert _trace_local(torch_log, tiling.exchange_until_stable_local_device, grid, script, CPU, max_rounds=3)[0] == rounds


def _ungated(log):
    """A gated trace as its fixed-rounds sibling must read: no gate, no copy, no reduce, refine_async for refine_dev."""
    out = []
    for who, call, args in log:
        if call in ("round_gate", "round_end", "copy_", "amax", "all_reduce"):
            continue
        out.append([who, "refine_async", []] if call == "refine_dev" else [who, call, args])
    return out


@pytest.mark.parametrize("grid", GRIDS, ids=_grid_name)
@pytest.mark.parametrize("rounds", BOUNDS)
def test_fixed_rounds_are_the_gated_rounds_without_the_gate(torch_log, grid, rounds):
    _, gated = _trace_local(torch_log, tiling.exchange_converged_local_device, grid, [0], CPU, max_rounds=rounds, bufs={})
    ret, fixed = _trace_local(torch_log, tiling.exchange_rounds_local_device, grid, [0], CPU, rounds=rounds, bufs={})
    assert ret == rounds and fixed == _ungated(gated)
    assert any(call == "round_gate" for _, call, _ in gated) and any(call == "amax" for _, call, _ in gated)

    gated = _trace_ranked(torch_log, tiling.exchange_converged_device, grid, [0], lambda: ((CPU, {}), dict(max_rounds=rounds, group="g")))
    fixed = _trace_ranked(torch_log, tiling.exchange_rounds_device, grid, [0], lambda: ((CPU, {}), dict(rounds=rounds, group="g")))
    assert sorted(fixed) == sorted(gated)
    for rank, (_, want) in gated.items():
        assert fixed[rank][0] == rounds and fixed[rank][1] == _ungated(want), rank
        assert any(call == "copy_" for _, call, _ in want) and any(call == "all_reduce" for _, call, _ in want)
