"""The ray-casting OGM as a plain statement: a second statement of registerLocObs / freeLocObs -> rayCastLoc, shared by
tests/test_independent_checks.py and tests/test_ray_cast_edges.py.

Written from pntcld_raycast.cu:11-117, ray_cast.h:57-144 and local_batch.h:114-126,250-258,303-350, not from the oracle: plain
Python loops, every float operation an np.float32 operation in the order the reference writes them (no fused multiply-add:
DESIGN.md deviation 4).  The pose has no rotation, so the sensor-to-map transform is a single float addition per coordinate and
does not go through anybody's SE3 code.

The pivot `pvt` is an argument: nothing below assumes that the sensor's cell lies inside the volume (clear() drops what falls
outside, the walk itself never looks at the volume), so a tile of a larger volume is stated by its pivot alone.

With `records` (a list) the statement also says, per point of the cloud, how its ray went: what the cases of tests/ray_cases.py
state their preconditions on.  A record is a dict:
  steps      number of steps walked (0: the point lies in the sensor's own cell, or is no usable point)
  stop       why the walk stopped: "occupied" (clearRayLoc found an OCCUPIED cell), "end" (cur == i1), "max_length", "len"
             (far > max_length / far > len, tested in that order), "own_cell", "unusable"
  ties       steps at which the smallest tMax was held by two or three axes when they were compared
  first_in   index of the first step whose cell lies inside the volume, -1 if there is none
  last_in    index of the last such step, -1 if there is none
  seg        which eighth of the ray's stay in the volume the stopping step's border crossing falls into (see _stay), -1 without
             a stay.  The stay is computed here in float64; the kernel computes its limits in float32 from tDelta, so a crossing
             next to a limit may belong to the neighbouring segment there: the eighths are approximate with respect to the
             kernel's own, good for "a stop in every segment, some first and some last of theirs", not for a claim about one ray
  seg_prev   the same for the step before it (-1: there is none), seg_next for the crossing that would have come next
"""
import numpy as np

_F = np.float32
FLT_MAX = np.finfo(np.float32).max
SEGS = 8                                          # the eighths `seg` counts in


def _pos2coord(p, w):
    return [int(np.floor(_F(_F(p[i]) / w) + _F(0.5))) for i in range(3)]          # floorf(p / w + 0.5f)


def _usable(g):
    """include/gie.h: a point with a non-finite coordinate or one beyond +-1e6 m is ignored (undefined in the reference)."""
    return all(abs(float(v)) <= 1.0e6 for v in g)                                   # (False for NaN)


def _stay(p0, d, ln, max_length, pvt, size, w):
    """[ts, te] in float64: the ray's stay in the volume grown by one cell on every side (cell centres pvt - 1 .. pvt + size, so
    borders at pvt - 1.5 and pvt + size + 0.5), with 2 w of slack in t at both ends, clipped to [0, min(len, max_length)]; None when
    the ray never comes there."""
    L = min(float(ln), float(max_length))
    tin, tout = 0.0, float("inf")
    for a in range(3):
        lo, hi = (pvt[a] - 1.5) * float(w), (pvt[a] + size[a] + 0.5) * float(w)
        if float(d[a]) != 0.0:
            ta, tb = (lo - float(p0[a])) / float(d[a]), (hi - float(p0[a])) / float(d[a])
            tin, tout = max(tin, min(ta, tb)), min(tout, max(ta, tb))
        elif float(p0[a]) < lo or float(p0[a]) > hi:
            return None
    ts, te = max(0.0, tin - 2.0 * float(w)), min(L, tout + 2.0 * float(w))
    return (ts, te) if ts < te else None


def _eighth(t, stay):
    if stay is None:
        return -1
    ts, te = stay
    return int(min(SEGS - 1, max(0, np.floor(SEGS * (float(t) - ts) / (te - ts)))))


def _raycast_second_statement(origin, pts, pvt, size, w, min_h, max_h, records=None):
    X, Y, Z = size
    count = np.zeros((Z, Y, X), np.int32)
    occ = np.zeros((Z, Y, X), bool)
    inside = lambda c: 0 <= c[0] < X and 0 <= c[1] < Y and 0 <= c[2] < Z
    glb = [[_F(_F(p[i]) + _F(origin[i])) for i in range(3)] for p in pts]
    for g in glb:                                                                   # registerLocObs
        if _usable(g) and g[2] >= min_h and g[2] <= max_h:
            c = [a - b for a, b in zip(_pos2coord(g, w), pvt)]
            if inside(c):
                occ[c[2], c[1], c[0]] = True
                count[c[2], c[1], c[0]] += 1

    def clear(cg):                                                                  # clearRayLoc on a global coordinate
        c = [a - b for a, b in zip(cg, pvt)]
        if inside(c):
            if occ[c[2], c[1], c[0]]:
                return False
            count[c[2], c[1], c[0]] -= 1
        return True                                                                 # (outside: type UNKNOWN, the add is dropped)

    max_length = _F(_F(_F(0.707) * _F(X)) * w)
    p0 = [_F(v) for v in origin]
    i0 = _pos2coord(p0, w)
    for p1 in glb:                                                                  # freeLocObs -> rayCastLoc
        rec = dict(steps=0, stop="unusable", ties=0, first_in=-1, last_in=-1, seg=-1, seg_prev=-1, seg_next=-1)
        if records is not None:
            records.append(rec)
        if not _usable(p1):
            continue
        i1 = _pos2coord(p1, w)
        clear(i0)
        if i0 == i1:
            rec["stop"] = "own_cell"
            continue
        d = [_F(p1[i] - p0[i]) for i in range(3)]
        ln = _F(np.sqrt(_F(_F(_F(d[0] * d[0]) + _F(d[1] * d[1])) + _F(d[2] * d[2]))))
        d = [_F(v / ln) for v in d]
        step, tmax, tdelta = [0] * 3, [FLT_MAX] * 3, [FLT_MAX] * 3
        cur = list(i0)
        for i in range(3):
            step[i] = 1 if d[i] > 0 else (-1 if d[i] < 0 else 0)
            if step[i]:
                border = _F(_F(_F(cur[i]) * w) + _F(_F(_F(step[i]) * w) * _F(0.5)))
                tmax[i] = _F(_F(border - p0[i]) / d[i])
                tdelta[i] = _F(w / _F(abs(d[i])))
        times = []                                                                  # the border crossing every step took
        while True:
            if tmax[0] < tmax[1]:
                dim = 0 if tmax[0] < tmax[2] else 2
            else:
                dim = 1 if tmax[1] < tmax[2] else 2
            lowest = min(tmax)
            rec["ties"] += int(sum(1 for t in tmax if t == lowest) > 1)
            times.append(tmax[dim])
            cur[dim] += step[dim]
            tmax[dim] = _F(tmax[dim] + tdelta[dim])
            if inside([a - b for a, b in zip(cur, pvt)]):
                if rec["first_in"] < 0:
                    rec["first_in"] = len(times) - 1
                rec["last_in"] = len(times) - 1
            if not clear(cur):
                rec["stop"] = "occupied"
                break
            if cur == i1:
                rec["stop"] = "end"
                break
            far = min(min(tmax[0], tmax[1]), tmax[2])
            if far > max_length or far > ln:
                rec["stop"] = "max_length" if far > max_length else "len"
                break
        rec["steps"] = len(times)
        if records is not None:
            stay = _stay(p0, d, ln, max_length, pvt, size, w)
            rec["seg"] = _eighth(times[-1], stay)
            rec["seg_prev"] = _eighth(times[-2], stay) if len(times) > 1 else -1
            rec["seg_next"] = _eighth(min(tmax), stay)
    lab = np.where(count > 0, 2, np.where(count < 0, 1, 0)).astype(np.int8)        # getAllocKeys: OCCUPIED / FREE / untouched
    return count, lab
