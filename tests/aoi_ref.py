"""Areas of interest of include/eve_hip.h (eve_gaze_aoi) in numpy float64: the contract the HIP kernel follows.  Every operation is
one IEEE double operation rounded on its own, in the order written here; only + - * / and comparisons occur, so the device equals
it bit for bit.  Per stream the frames are walked in time order with a carried state row of 16 doubles (STATE below), so any split
of a clip into chunks gives the bits of one pass.

    out = run(spec, pog, shapes, state, table, trans, visits, count, dropped, frame_time=, valid=, valid_key=, fixation_id=,
              fixating=, lengths=, reset=, flush=)

spec: anything with fps and max_gap_s (eve_amd.AoiSpec; Spec below is a plain stand-in).  pog [B, T, 2] float32; shapes float32
[B, A, 36] or [B, T, A, 36] (one table per frame); state float64 [B, 16], table float64 [B, A + 1, 8], trans int32 [B, A + 1, A],
visits float64 [B, V, 8], count and dropped int32 [B]: UPDATED IN PLACE.  -> {'id': int32 [B, T], 'mask': int64 [B, T], 'visit_ms':
float32 [B, T]}."""
import numpy as np

STATE_DOUBLES = 16
ROW = 36                                                 # floats per AOI: kind, n, two reserved, 32 coordinates
MAX_AOIS = 64
# the state row: an all-zero row is a fresh stream, so "none" is 0 and an AOI index or a fixation id is stored as id + 1
TICKS, HAS_PREV, T_PREV, PREV_AOI, OPEN, V_AOI, T_ENTER, T_LAST, V_SAMPLES, V_FIXATIONS, V_INDEX, NEXT_INDEX, LAST_AOI, FIX_ID, FIX_AOI = range(15)
# the columns of a table row
DWELL, SAMPLES, VISITS, T_FIRST_ENTRY, TAB_T_LAST, FIXATIONS, T_FIRST_FIXATION = range(7)
F64 = np.float64


class Spec(object):
    def __init__(self, fps=None, max_gap_s=0.075):
        self.fps, self.max_gap_s = fps, max_gap_s


def fresh(B, A, capacity):
    """-> (state, table, trans, visits, count, dropped) of B streams that have seen nothing."""
    return (np.zeros((B, STATE_DOUBLES)), np.zeros((B, A + 1, 8)), np.zeros((B, A + 1, A), dtype=np.int32), np.zeros((B, capacity, 8)),
            np.zeros(B, dtype=np.int32), np.zeros(B, dtype=np.int32))


def contains(row, x, y):
    """Does the AOI row (36 float32) contain the point (x, y), both float64?"""
    r = np.asarray(row, dtype=np.float32).astype(F64)
    kind = r[0]
    if kind == 1.0:                                      # rectangle (x0, y0, x1, y1): half open
        if not np.isfinite(r[4:8]).all():
            return False
        return bool(r[4] <= x and x < r[6] and r[5] <= y and y < r[7])
    if kind == 2.0:                                      # ellipse (cx, cy, rx, ry)
        if not np.isfinite(r[4:8]).all() or not (r[6] > 0.0 and r[7] > 0.0):
            return False
        u = (x - r[4]) / r[6]
        v = (y - r[5]) / r[7]
        return bool(u * u + v * v <= 1.0)
    if kind == 3.0:                                      # polygon, even-odd
        if not (r[1] >= 3.0 and r[1] <= 16.0) or r[1] != np.floor(r[1]):
            return False
        n = int(r[1])
        if not np.isfinite(r[4:4 + 2 * n]).all():
            return False
        inside = False
        for i in range(n):
            j = n - 1 if i == 0 else i - 1
            xi, yi, xj, yj = r[4 + 2 * i], r[5 + 2 * i], r[4 + 2 * j], r[5 + 2 * j]
            if (yi > y) != (yj > y) and x < (xj - xi) * (y - yi) / (yj - yi) + xi:
                inside = not inside
        return inside
    return False


def hit_mask(rows, x, y):
    """-> the Python int whose bit a is set iff rows[a] contains (x, y)."""
    m = 0
    for a in range(len(rows)):
        if contains(rows[a], x, y):
            m |= 1 << a
    return m


def lowest_bit(m):
    return -1 if m == 0 else (m & -m).bit_length() - 1


def close_visit(row, visits, count, dropped, b):
    if row[OPEN] == 0:
        return
    row[OPEN] = 0.0
    row[LAST_AOI] = row[V_AOI]
    if count[b] < visits.shape[1]:
        visits[b, count[b]] = (row[V_AOI] - 1.0, row[T_ENTER], row[T_LAST], row[V_SAMPLES], row[V_FIXATIONS], row[V_INDEX], 0.0, 0.0)
        count[b] += 1
    else:
        dropped[b] += 1


def run(spec, pog, shapes, state, table, trans, visits, count, dropped, frame_time=None, valid=None, valid_key=None, fixation_id=None,
        fixating=None, lengths=None, reset=None, flush=None):
    pog = np.asarray(pog, dtype=np.float32)
    B, T = pog.shape[:2]
    A = table.shape[1] - 1
    assert (fixation_id is None) == (fixating is None)
    out = {'id': np.full((B, T), -2, dtype=np.int32), 'mask': np.zeros((B, T), dtype=np.int64), 'visit_ms': np.zeros((B, T), dtype=np.float32)}
    fps = None if spec.fps is None else F64(spec.fps)
    max_gap = F64(spec.max_gap_s)
    with np.errstate(all='ignore'):
        for b in range(B):
            row, tab, tr = state[b], table[b], trans[b]
            if reset is not None and reset[b] != 0:
                close_visit(row, visits, count, dropped, b)
                keep = row[NEXT_INDEX]
                row[:] = 0.0
                row[NEXT_INDEX] = keep
            n_frames = T if lengths is None else min(max(int(lengths[b]), 0), T)
            ticks0 = row[TICKS]
            for f in range(n_frames):
                tt = F64(frame_time[b, f]) if frame_time is not None else (ticks0 + F64(f)) / fps
                x, y = F64(pog[b, f, 0]), F64(pog[b, f, 1])
                ok = (valid is None or valid[b, f] != 0) and (valid_key is None or valid_key[b, f] != 0) and \
                    bool(np.isfinite(x)) and bool(np.isfinite(y)) and bool(np.isfinite(tt))
                if not ok or (row[HAS_PREV] != 0 and not tt > row[T_PREV]):
                    continue                                     # not a sample: nothing moves
                dt = tt - row[T_PREV]
                restart = row[HAS_PREV] == 0 or dt > max_gap
                rows = shapes[b, f] if shapes.ndim == 4 else shapes[b]
                m = hit_mask(rows, x, y)
                a = lowest_bit(m)
                if restart:
                    close_visit(row, visits, count, dropped, b)
                elif row[OPEN] != 0 and F64(a + 1) != row[V_AOI]:
                    close_visit(row, visits, count, dropped, b)
                if a >= 0:
                    if row[OPEN] == 0:
                        row[OPEN], row[V_AOI], row[T_ENTER], row[V_SAMPLES], row[V_FIXATIONS] = 1.0, F64(a + 1), tt, 0.0, 0.0
                        row[V_INDEX] = row[NEXT_INDEX]
                        row[NEXT_INDEX] = row[NEXT_INDEX] + 1.0
                        if tab[a, VISITS] == 0:
                            tab[a, T_FIRST_ENTRY] = tt
                        tab[a, VISITS] += 1.0
                        tr[A if row[LAST_AOI] == 0 else int(row[LAST_AOI]) - 1, a] += 1
                    else:
                        tab[a, DWELL] = tab[a, DWELL] + dt
                    row[V_SAMPLES] += 1.0
                    row[T_LAST] = tt
                    tab[a, SAMPLES] += 1.0
                    tab[a, TAB_T_LAST] = tt
                    out['visit_ms'][b, f] = np.float32(F64(1000.0) * (tt - row[T_ENTER]))
                    if fixation_id is not None and fixating[b, f] != 0 and fixation_id[b, f] >= 0 and \
                            (F64(int(fixation_id[b, f]) + 1) != row[FIX_ID] or F64(a + 1) != row[FIX_AOI]):
                        if tab[a, FIXATIONS] == 0:
                            tab[a, T_FIRST_FIXATION] = tt
                        tab[a, FIXATIONS] += 1.0
                        row[V_FIXATIONS] += 1.0
                        row[FIX_ID], row[FIX_AOI] = F64(int(fixation_id[b, f]) + 1), F64(a + 1)
                else:
                    tab[A, SAMPLES] += 1.0
                    if not restart and row[PREV_AOI] == 0:
                        tab[A, DWELL] = tab[A, DWELL] + dt
                row[HAS_PREV], row[T_PREV], row[PREV_AOI] = 1.0, tt, F64(a + 1)
                out['id'][b, f] = a
                out['mask'][b, f] = np.array(m, dtype=np.uint64).astype(np.int64)
            row[TICKS] = ticks0 + F64(n_frames)
            if flush is not None and flush[b] != 0:
                close_visit(row, visits, count, dropped, b)
    return out


# ---------------------------------------------------------------------------------------------------------------- building tables
def rect(x0, y0, x1, y1):
    return _row(1, 0, [x0, y0, x1, y1])


def ellipse(cx, cy, rx, ry):
    return _row(2, 0, [cx, cy, rx, ry])


def polygon(points):
    return _row(3, len(points), [c for p in points for c in p])


def disabled():
    return np.zeros(ROW, dtype=np.float32)


def _row(kind, n, coords):
    r = np.zeros(ROW, dtype=np.float32)
    r[0], r[1] = kind, n
    r[4:4 + len(coords)] = coords
    return r
