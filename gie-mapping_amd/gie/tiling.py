"""Spatial sharding of a large local volume over the GPUs of one node.

A volume of `grid` voxels is cut into block-aligned tiles, one per rank; rank r owns the voxels
(and the global voxel blocks) of its tile.  After every map update the tiles exchange the
one-voxel layers on their shared faces (export -> transfer -> import as ghost voxels -> refine);
the variants below differ in where the tiles live (one process / one rank each) and in who
orders the steps (the host, or the mappers' own streams).
"""
import numpy as np


def tile_grid(world_size):
    """Tiles per axis (tx, ty, tz) for a world size that is a power of two: 1→(1,1,1), 2→(2,1,1),
    4→(2,2,1), 8→(2,2,2), …"""
    if world_size < 1 or world_size & (world_size - 1):
        raise ValueError("world_size must be a power of two")
    t = [1, 1, 1]
    a = 0
    while t[0] * t[1] * t[2] < world_size:
        t[a] *= 2
        a = (a + 1) % 3
    return tuple(t)


def tile_of_rank(rank, world_size, tile_size):
    """Origin (in voxels, relative to the large volume's corner) and size of rank's tile."""
    tx, ty, tz = tile_grid(world_size)
    ix, iy, iz = rank % tx, (rank // tx) % ty, rank // (tx * ty)
    size = tuple(int(s) for s in tile_size)
    if any(s % 8 for s in size):
        raise ValueError("tiles must be aligned to the 8-voxel blocks")
    return (ix * size[0], iy * size[1], iz * size[2]), size


def tile_offset_voxels(rank, world_size, tile_size):
    """Integer offset (voxels) of the tile centre from the centre of the whole volume — the
    argument of Mapper.set_tile_offset when all tiles share one sensor pose."""
    origin, size = tile_of_rank(rank, world_size, tile_size)
    t = tile_grid(world_size)
    return tuple(int(origin[i] + size[i] // 2 - (t[i] * size[i]) // 2) for i in range(3))


def tile_centre_offset(rank, world_size, tile_size, voxel_width):
    """Metric offset of the tile centre from the centre of the whole volume: the pose a rank
    feeds its mapper is the shared sensor pose shifted by this."""
    origin, size = tile_of_rank(rank, world_size, tile_size)
    t = tile_grid(world_size)
    whole = np.array([t[i] * size[i] for i in range(3)], dtype=np.float64)
    centre = np.array(origin, dtype=np.float64) + 0.5 * np.array(size, dtype=np.float64)
    return tuple(((centre - 0.5 * whole) * voxel_width).tolist())


def aggregate(dist, seconds, voxels_per_rank, steps):
    """Whole-job throughput [Mvoxels/s] from the slowest rank's time (max-reduce)."""
    import torch
    t = torch.tensor([seconds], dtype=torch.float64)
    if dist is not None and dist.is_initialized():
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        world = dist.get_world_size()
    else:
        world = 1
    t_max = float(t.item())
    return world * voxels_per_rank * steps / t_max / 1e6, t_max


# face = 2*axis + side (include/gie.h); the neighbour across my face f imports my layer as its face f^1
def neighbours(rank, world_size):
    """{face: neighbour rank} for the tiles that exist around `rank`."""
    t = tile_grid(world_size)
    idx = [rank % t[0], (rank // t[0]) % t[1], rank // (t[0] * t[1])]
    out = {}
    for axis in range(3):
        for side in (0, 1):
            j = list(idx)
            j[axis] += 1 if side else -1
            if 0 <= j[axis] < t[axis]:
                out[2 * axis + side] = j[0] + t[0] * (j[1] + t[1] * j[2])
    return out


# Every exchange function below expects its mappers in the middle of a TILED map update — Mapper.update(..., tiled=True) or
# Mapper.step_begin_tiled(): fuse, batch EDT and the first half of the merge are done, the face layers hold this update's
# Mark-time state.  Round 0 exports / imports them and finishes the merge (gie_merge_end: obtainFrontiers + waves with fresh
# ghosts); the rounds after it are export / import / gie_refine.
#
# Each of them picks a topology (_InProcess / _Ranked: where the tiles are, and so what "move" means), one of the topology's three
# layer forms (host arrays, per-face device tensors ordered by the host, all faces in one call ordered on the mappers' streams)
# and a stop rule (_until_stable, or _enqueued with or without the device-side gate).  The stop rule loops over _round.

def _round(exchange, k, refine):
    """Round k, the Python side of TiledMapper::round (host/gie_tiled.hpp): `exchange(k)` exports the shared faces, moves them and
    imports them, and yields each mapper once its ghosts are in; round 0 then finishes that mapper's merge, every later round
    refines.  Returns what the refine calls returned, by tile."""
    return [m.merge_end() if k == 0 else refine(r, m) for r, m in enumerate(exchange(k))]


def _until_stable(topo, exchange, max_rounds):
    """Stop rule "until no tile seeded anything": the host reads refine() every round (which synchronises the mapper) and the
    topology totals the counts.  Returns the refinement rounds run."""
    for k in range(max_rounds + 1):
        seeded = _round(exchange, k, lambda r, m: m.refine())
        if k and topo.total(seeded) == 0:
            break
    return k


def _enqueued(topo, bufs, rounds, gated):
    """Stop rules with nobody waiting for the host, over the all-faces form: `rounds` refinement rounds enqueued back to back
    (refine_async).  gated=True are the same rounds gated on the device: gie_round_gate before every export, gie_refine_dev leaves
    what each tile seeded in its "changed" word, the topology max-reduces those into "go" — the gate of the NEXT round —, and
    gie_round_end closes the update."""
    import torch
    topo.buffers(bufs)
    _stream_state(topo, bufs, gated)
    if gated:
        go, changed, esz = bufs["go"].data_ptr(), bufs["changed"].data_ptr(), bufs["changed"].element_size()
    with torch.cuda.stream(bufs["stream"]):               # a rank's transfers and reduce go to the current stream; None: stay
        for k in range(rounds + 1):
            if gated:
                gate, refine = (lambda m: m.round_gate(go if k > 1 else None)), (lambda r, m: m.refine_dev(changed + r * esz))
            else:
                gate, refine = None, (lambda r, m: m.refine_async())
            _round(lambda k: topo.all_faces(bufs, gate), k, refine)
            if gated and k:
                topo.reduce_changed(bufs)
        if gated:
            topo.round_end(bufs)


def _local_face_buffers(mappers, world, device, bufs):
    """One tensor per (exporting tile, face), allocated once and kept in `bufs`: only the mappers' own streams touch
    them, so their lifetime must not hang on torch's allocator (a tensor dropped after round k could be handed out
    again while a neighbour's import of round k is still reading it)."""
    import torch
    if "layers" not in bufs:
        bufs["layers"] = {(r, face): torch.empty(m.halo_count(face) * 20, dtype=torch.uint8, device=device)
                          for r, m in enumerate(mappers) for face in neighbours(r, world)}
    return bufs["layers"]


def _stream_state(topo, bufs, gated):
    """The stream and event state of the stream-ordered forms, built on first use: every mapper's own stream as a torch stream
    ("streams"), the events behind the last round's imports ("imported": an exporter may rewrite its layers only after them) and
    the stream that is current while the rounds are enqueued ("stream": a rank's own, for its transfers and its all-reduce; none
    in process).  Gated rounds add one "changed" word per tile, the "go" word they are max-reduced into and, in process, the
    "side" stream that reduction runs on.  With device "cpu" (emulated mappers) the words are host memory and every stream is
    None: no events."""
    import torch
    cuda = getattr(topo.device, "type", str(topo.device)) == "cuda"
    if "streams" not in bufs:
        bufs["streams"] = [torch.cuda.ExternalStream(m.stream_handle(), device=topo.device) if cuda else None for m in topo.mappers]
        bufs["stream"] = bufs["streams"][0] if isinstance(topo, _Ranked) else None
        bufs["imported"] = []
    if gated and "go" not in bufs:
        bufs["side"] = torch.cuda.Stream(device=topo.device) if cuda and bufs["stream"] is None else None
        bufs["changed"] = torch.zeros(len(topo.mappers), dtype=torch.int32, device=topo.device)
        bufs["go"] = torch.ones(1, dtype=torch.int32, device=topo.device)


class _InProcess:
    """All tiles live in this process: "move" hands a layer, or the pointer of its tensor, to face f ^ 1 of the neighbour."""

    def __init__(self, mappers, grid, device=None):
        self.mappers, self.device, self.world = mappers, device, grid[0] * grid[1] * grid[2]
        assert self.world == len(mappers)
        self.nbs = [neighbours(r, self.world) for r in range(self.world)]
        self.go_ready = []

    def total(self, seeded):
        return sum(seeded)

    def sync(self):
        for m in self.mappers:
            m.sync()

    def buffers(self, bufs):
        """self.out[r] / self.inp[r]: {face: pointer} of the layers tile r exports, and of its neighbours' layers it imports."""
        lay = _local_face_buffers(self.mappers, self.world, self.device, bufs)
        self.out = [{face: lay[(r, face)].data_ptr() for face in nbs} for r, nbs in enumerate(self.nbs)]
        self.inp = [{face: lay[(nb, face ^ 1)].data_ptr() for face, nb in nbs.items()} for nbs in self.nbs]

    def host_layers(self, sparse, sent):
        layers = {}
        for r, m in enumerate(self.mappers):
            for face, nb in self.nbs[r].items():
                layers[(nb, face ^ 1)] = m.halo_export_sparse(face) if sparse else m.halo_export(face)
                if sent is not None:
                    sent.append(layers[(nb, face ^ 1)].nbytes)
        for (r, face), layer in layers.items():
            m = self.mappers[r]
            (m.halo_import_sparse if sparse else m.halo_import)(face, layer)
        yield from self.mappers

    def face_tensors(self, k):
        for m, out in zip(self.mappers, self.out):
            for face, p in out.items():
                m.halo_export_dev(face, p)
        self.sync()
        for m, inp in zip(self.mappers, self.inp):
            for face, p in inp.items():
                m.halo_import_dev(face, p)
        for m in self.mappers:
            yield m                                       # refine() synchronises its mapper, merge_end does not:
            if k == 0:
                m.sync()                                  # either way the layers are free again

    def _record(self, stream):
        import torch
        if stream is not None:
            ev = torch.cuda.Event()
            ev.record(stream)
            return ev

    def _wait(self, stream, evs):
        if stream is not None:
            for ev in evs:
                stream.wait_event(ev)

    def all_faces(self, bufs, gate):
        streams, evs, done = bufs["streams"], [], []
        for r, m in enumerate(self.mappers):
            self._wait(streams[r], bufs["imported"] + self.go_ready)   # the layers of the round before have been read; this round's gate is final
            if gate:
                gate(m)
            m.halo_export_all_dev(self.out[r])
            evs.append(self._record(streams[r]))
        for r, m in enumerate(self.mappers):
            self._wait(streams[r], evs)                   # the neighbour's stream waits for the exporter's instead of a transfer
            m.halo_import_all_dev(self.inp[r])
            done.append(self._record(streams[r]))
            yield m
        bufs["imported"] = done

    def reduce_changed(self, bufs):
        """The all-reduce(max): one reduction on the side stream, behind every mapper's refinement, that everybody's next round
        (and round_end) waits for."""
        import torch
        side = bufs["side"]
        for stream in bufs["streams"]:
            self._wait(side, [self._record(stream)])      # "refined": nothing follows refine_dev on a mapper's stream in this round
        with torch.cuda.stream(side):
            torch.amax(bufs["changed"], dim=0, keepdim=True, out=bufs["go"])
        self.go_ready = [self._record(side)]

    def round_end(self, bufs):
        for stream, m in zip(bufs["streams"], self.mappers):
            self._wait(stream, self.go_ready)
            m.round_end(bufs["go"].data_ptr())


class _Ranked:
    """One tile per rank: "move" is batch_isend_irecv over the P2P ops of the shared faces, in sorted face order."""

    def __init__(self, mapper, dist, rank, world_size, group, device):
        self.mappers, self.dist, self.group, self.device = [mapper], dist, group, device
        self.nbs = sorted(neighbours(rank, world_size).items())

    def total(self, seeded):
        import torch
        n = torch.tensor(seeded, dtype=torch.int64, device=self.device)
        self.dist.all_reduce(n, op=self.dist.ReduceOp.SUM, group=self.group)
        return int(n.item())

    def ops(self, pairs):
        """The P2P op list over (send tensor, receive tensor) per face of self.nbs; a tensor without elements stays out of it."""
        d, ops = self.dist, []
        for (snd, rcv), (_, nb) in zip(pairs, self.nbs):
            if snd.numel():
                ops.append(d.P2POp(d.isend, snd, nb, group=self.group))
            if rcv.numel():
                ops.append(d.P2POp(d.irecv, rcv, nb, group=self.group))
        return ops

    def move(self, ops, host_waits=False):
        import torch
        if ops:
            for w in self.dist.batch_isend_irecv(ops):
                w.wait()                                  # stream-level on RCCL: the current stream waits for the transfer
            if host_waits:
                torch.cuda.synchronize(self.device)

    def buffers(self, bufs, sparse=False):
        """Everything that does not change from round to round, once: bufs[face] = the (send, receive) tensors of a shared face,
        "out" / "in" their pointers and "ops" the P2P op list over them.  sparse: entries of 24 bytes instead of records of 20,
        and bufs[("count", face)] = the (sent, received) entry counts."""
        import torch
        if "ops" in bufs:
            return
        for face, _ in self.nbs:
            n = self.mappers[0].halo_count(face) * (24 if sparse else 20)
            bufs[face] = (torch.empty(n, dtype=torch.uint8, device=self.device), torch.empty(n, dtype=torch.uint8, device=self.device))
            if sparse:
                bufs[("count", face)] = (torch.zeros(1, dtype=torch.int32, device=self.device), torch.zeros(1, dtype=torch.int32, device=self.device))
        bufs["out"] = {face: bufs[face][0].data_ptr() for face, _ in self.nbs}
        bufs["in"] = {face: bufs[face][1].data_ptr() for face, _ in self.nbs}
        bufs["ops"] = self.ops(bufs[face] for face, _ in self.nbs)

    def host_layers(self, sparse):
        import torch
        from .mapper import HALO_DTYPE, HALO_ENTRY_DTYPE
        m, dtype = self.mappers[0], HALO_ENTRY_DTYPE if sparse else HALO_DTYPE
        lays = [m.halo_export_sparse(face) if sparse else m.halo_export(face) for face, _ in self.nbs]
        snd = [torch.from_numpy(lay.view(np.uint8).copy()).to(self.device) for lay in lays]
        if sparse:                                        # the neighbours tell each other the entry counts first
            cs = [torch.tensor([lay.shape[0]], dtype=torch.int64, device=self.device) for lay in lays]
            cr = [torch.zeros(1, dtype=torch.int64, device=self.device) for lay in lays]
            self.move(self.ops(zip(cs, cr)))
            rcv = [torch.empty(int(c.item()) * dtype.itemsize, dtype=torch.uint8, device=self.device) for c in cr]
        else:
            rcv = [torch.empty_like(t) for t in snd]
        self.move(self.ops(zip(snd, rcv)))
        for (face, _), r in zip(self.nbs, rcv):
            (m.halo_import_sparse if sparse else m.halo_import)(face, r.cpu().numpy().view(dtype))
        yield m

    def face_tensors(self, bufs, sparse):
        m, ops = self.mappers[0], bufs["ops"]
        for face, _ in self.nbs:
            if sparse:
                m.halo_export_sparse_dev(face, bufs["out"][face], bufs[("count", face)][0].data_ptr())
            else:
                m.halo_export_dev(face, bufs["out"][face])
        m.sync()                                          # export kernels ran on the mapper's own stream
        if sparse:                                        # the counts first, read by the host; then only that many entries
            self.move(self.ops(bufs[("count", face)] for face, _ in self.nbs), host_waits=True)
            ops = self.ops((bufs[face][i][:int(bufs[("count", face)][i].item()) * 24] for i in (0, 1)) for face, _ in self.nbs)
        self.move(ops, host_waits=True)
        for face, _ in self.nbs:
            if sparse:
                m.halo_import_sparse_dev(face, bufs["in"][face], bufs[("count", face)][1].data_ptr())
            else:
                m.halo_import_dev(face, bufs["in"][face])
        yield m

    def all_faces(self, bufs, gate):
        m = self.mappers[0]
        if gate:
            gate(m)
        m.halo_export_all_dev(bufs["out"])
        self.move(bufs["ops"])                            # on the mapper's stream: the import below is ordered behind the transfer
        m.halo_import_all_dev(bufs["in"])
        yield m

    def reduce_changed(self, bufs):
        bufs["go"].copy_(bufs["changed"])
        self.dist.all_reduce(bufs["go"], op=self.dist.ReduceOp.MAX, group=self.group)

    def round_end(self, bufs):
        self.mappers[0].round_end(bufs["go"].data_ptr())


def exchange_until_stable_local(mappers, grid, max_rounds=64, sparse=False, sent=None):
    """All tiles live in this process (tests, single-GPU checks): export every shared face, hand
    it to the neighbour, finish the merge (round 0) or refine, repeat until no tile seeded anything.
    Returns the refinement rounds run.  sparse=True: the layers travel in their sparse form (known voxels only,
    gie_halo_export_sparse / gie_halo_import_sparse); `sent` (a list) collects the bytes of every layer handed over."""
    topo = _InProcess(mappers, grid)
    return _until_stable(topo, lambda k: topo.host_layers(sparse, sent), max_rounds)


def exchange_until_stable_local_device(mappers, grid, device, max_rounds=64, bufs=None):
    """In-process variant of the device-resident exchange (all tiles on one GPU): the export
    kernel of one mapper writes the tensor the import kernel of its neighbour reads."""
    topo = _InProcess(mappers, grid, device)
    topo.buffers({} if bufs is None else bufs)
    return _until_stable(topo, topo.face_tensors, max_rounds)


def exchange_until_stable_device(mapper, dist, rank, world_size, device, bufs=None, max_rounds=64, group=None, sparse=False):
    """Device-resident form of exchange_until_stable for backend "nccl" (RCCL over xGMI): the
    face layers are written by the export kernel straight into the send tensors and read by the
    import kernel from the receive tensors; nothing crosses PCIe except the seed count.
    sparse=True: gie_halo_export_sparse_dev compacts the known voxels of a layer; the neighbours exchange the entry counts
    (one more small batch and one host read per round — this form waits for the host anyway), then only that many entries."""
    topo, bufs = _Ranked(mapper, dist, rank, world_size, group, device), {} if bufs is None else bufs
    topo.buffers(bufs, sparse)
    return _until_stable(topo, lambda k: topo.face_tensors(bufs, sparse), max_rounds)


def exchange_rounds_device(mapper, dist, rank, world_size, device, bufs, rounds=1, group=None):
    """A fixed number of exchange rounds, ordered ON THE MAPPER'S STREAM: export kernels, the RCCL
    send / receive of the face layers, ghost import and refinement are enqueued back to back and
    the host never waits (no seed count comes back, so there is no convergence test: information
    crosses one tile boundary per round, the rest follows with the next map update)."""
    _enqueued(_Ranked(mapper, dist, rank, world_size, group, device), bufs, rounds, gated=False)
    return rounds


def exchange_converged_device(mapper, dist, rank, world_size, device, bufs, max_rounds=4, group=None):
    """rounds "until no GPU changed", ordered ON THE MAPPER'S STREAM with nobody waiting for the host.  Round 0 finishes
    the merge with this update's ghosts.  Then at most `max_rounds` refinement rounds are enqueued back to back: export, RCCL send /
    receive of the face layers, import, gie_refine_dev — which leaves the number of voxels it seeded in a device word —, and a 4-byte
    all-reduce(max) of that word over the ranks on the same stream.  The result gates the NEXT round (gie_round_gate): once no tile
    changed, every kernel of the remaining rounds returns at once (the transfers still run: a collective cannot be skipped by one
    side).  gie_round_end counts an update whose last all-reduce was still non-zero as unconverged (Mapper.round_stats()): the
    bound was too small — tests hold the bench's bound against the tiled oracle.  Works on the CPU too (emulated mappers, gloo):
    `device` "cpu", the "device words" are then host memory.
    Returns nothing the host could know without waiting: the rounds that ran are in round_stats()."""
    _enqueued(_Ranked(mapper, dist, rank, world_size, group, device), bufs, max_rounds, gated=True)


def exchange_converged_local_device(mappers, grid, device, max_rounds=4, bufs=None):
    """exchange_converged_device with all tiles in this process (one GPU, or emulated mappers with device "cpu"): the neighbour's
    stream waits for an event on the exporter's stream instead of an RCCL transfer, and the all-reduce(max) of the "changed" words
    is one reduction on a side stream that waits for every mapper's refinement and that every mapper's next round waits for."""
    topo = _InProcess(mappers, grid, device)
    _enqueued(topo, {} if bufs is None else bufs, max_rounds, gated=True)
    if bufs is None:                                      # nobody keeps the layers alive after the call: finish before returning
        topo.sync()


def exchange_rounds_local_device(mappers, grid, device, rounds=1, bufs=None):
    """The same stream-ordered rounds with all tiles in this process (one GPU): the neighbour's
    stream waits for an event on the exporter's stream instead of an RCCL transfer.  The face layers
    are allocated once (`bufs`, kept by the caller across calls); an exporter rewrites its layers only
    after every import of the round before has finished (events recorded behind the imports)."""
    topo = _InProcess(mappers, grid, device)
    _enqueued(topo, {} if bufs is None else bufs, rounds, gated=False)
    if bufs is None:                                      # nobody keeps the layers alive after the call: finish before returning
        topo.sync()
    return rounds


def exchange_until_stable(mapper, dist, rank, world_size, device=None, max_rounds=64, group=None, sparse=False):
    """One tile per rank: face layers travel with torch.distributed point-to-point ops (RCCL over
    xGMI with backend "nccl", gloo on CPU); a 1-int all-reduce(sum) of the seed counts is the
    convergence test.  Returns the refinement rounds run.  sparse=True: only the known voxels of a layer travel
    (gie_halo_export_sparse); the neighbours tell each other the entry counts first, so a round is two batches."""
    topo = _Ranked(mapper, dist, rank, world_size, group, device)
    return _until_stable(topo, lambda k: topo.host_layers(sparse), max_rounds)


def init_transport(torch, dist, rank, world_size, device, want="nccl", preflight_timeout_s=120):
    """The process group(s) of a tiled run.  The control plane (barriers, timing reductions, the agreement below) is always a
    gloo group — it exists wherever torch.distributed does.  The data plane is RCCL (backend "nccl", over xGMI) when `want`
    says so AND a PRE-FLIGHT on every rank succeeds: group creation, one all-reduce and one ring send / receive of a device
    buffer, checked.  Every rank then learns over gloo whether ANY rank failed, so that all of them take the same path: RCCL, or
    the face layers staged through the host over gloo with the reason recorded.  Returns {"backend", "group", "note"}: `group`
    is what the exchange functions above take (None = the default gloo group)."""
    import datetime
    if not dist.is_initialized():
        dist.init_process_group("gloo", timeout=datetime.timedelta(seconds=900))
    info = {"backend": "gloo", "group": None, "note": None}
    if want != "nccl" or world_size < 2:
        return info
    err, g = None, None
    try:
        g = dist.new_group(backend="nccl", timeout=datetime.timedelta(seconds=preflight_timeout_s))
        t = torch.ones(1, device=device)
        dist.all_reduce(t, group=g)
        snd = torch.full((4096,), rank % 251, dtype=torch.uint8, device=device)
        rcv = torch.empty_like(snd)
        ops = [dist.P2POp(dist.isend, snd, (rank + 1) % world_size, group=g), dist.P2POp(dist.irecv, rcv, (rank - 1) % world_size, group=g)]
        for w in dist.batch_isend_irecv(ops):
            w.wait()
        torch.cuda.synchronize(device)
        if int(t.item()) != world_size or int(rcv[0].item()) != ((rank - 1) % world_size) % 251 or int(rcv[-1].item()) != int(rcv[0].item()):
            err = "pre-flight data mismatch"
    except Exception as e:            # noqa: BLE001 — whatever RCCL raises (no xGMI, IPC refused, a peer that never arrives) is a reason to fall back
        err = "%s: %s" % (type(e).__name__, str(e).splitlines()[0][:200] if str(e) else "")
    flag = torch.tensor([1 if err else 0], dtype=torch.int32)
    dist.all_reduce(flag, op=dist.ReduceOp.MAX)          # over gloo: one answer for everybody
    if int(flag.item()) == 0:
        info.update(backend="nccl", group=g)
    else:
        info["note"] = "RCCL pre-flight failed (%s): face layers staged through the host over gloo" % (err or "on another rank")
    return info
