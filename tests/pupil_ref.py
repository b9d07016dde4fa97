"""Pupillometry of include/eve_hip.h (eve_pupil_track) in numpy float64: the contract the HIP kernel follows.  Every operation is one
IEEE double operation rounded on its own, in the order written here; only + - * /, abs and comparisons occur, so the device equals
it bit for bit.  Per stream the frames are walked in time order with a carried state row of 32 doubles (STATE below), so any split
of a clip into chunks gives the bits of one pass.

    out = run(spec, left, right, state, table, light, store, count, dropped, eye_valid=, frame_time=, lengths=, reset=, flush=,
              luminance=, baseline_mark=)

spec: anything with the fields of eve_amd.PupilSpec but the name (Spec below is a plain stand-in).  left, right [B, T] float32;
state float64 [B, 32], table float64 [B, 24], light float64 [B, 4] (only read), store float64 [B, capacity, 8], count and dropped
int32 [B]: UPDATED IN PLACE.  -> a dict of KEYS."""
import numpy as np

STATE_DOUBLES = 32
TABLE_DOUBLES = 24
KEYS = ('mm', 'raw_mm', 'velocity', 'change_mm', 'change_pct', 'valid', 'eye_used', 'eye_reason', 'event')
# the state row: an all-zero row is a fresh stream
(TICKS, HAS_PREV, T_PREV, DF, LAST_IDX, HAS_L, T_L, V_L, HAS_R, T_R, V_R, HAS_OFF, OFF, HAS_LUM, T_LUM, LF, HAS_BASE, BASE, B_N, B_D0, B_SUM,
 PREV_MARK, EP_OPEN, EP_PHASE, EP_T_START, EP_T_END, EP_D_START, EP_D_END, EP_PEAK, EP_SAMPLES, EP_LF, EP_COUNT) = range(32)
# the table row
COVERED, LOST, BOTH, LEFT, RIGHT = range(5)
REJ = 5                                                  # REJ + 3 * eye + (0 not finite, 1 range, 2 speed)
D0, S1, S2, MIN, MAX, N, X0, Y0, SX, SY, SXX, SXY, SYY = range(11, 24)
WITHHELD, NOT_FINITE, RANGE, SPEED = 1, 2, 4, 8          # eye_reason
F64 = np.float64
TWO_PI = F64(6.283185307179586)


class Spec(object):
    def __init__(self, fps=None, min_mm=1.5, max_mm=9.0, max_speed_mm_s=10.0, max_gap_s=0.25, offset_rate=0.125, cutoff_hz=4.0, light_tau_s=0.5,
                 baseline_tau_s=None, dilate_mm_s=0.25, constrict_mm_s=0.25, min_amplitude_mm=0.0625):
        self.fps, self.min_mm, self.max_mm, self.max_speed_mm_s, self.max_gap_s, self.offset_rate = fps, min_mm, max_mm, max_speed_mm_s, max_gap_s, offset_rate
        self.cutoff_hz, self.light_tau_s, self.baseline_tau_s = cutoff_hz, light_tau_s, baseline_tau_s
        self.dilate_mm_s, self.constrict_mm_s, self.min_amplitude_mm = dilate_mm_s, constrict_mm_s, min_amplitude_mm


def fresh(B, capacity):
    """-> (state, table, light, store, count, dropped) of B streams that have seen nothing."""
    return (np.zeros((B, STATE_DOUBLES)), np.zeros((B, TABLE_DOUBLES)), np.zeros((B, 4)), np.zeros((B, capacity, 8)),
            np.zeros(B, dtype=np.int32), np.zeros(B, dtype=np.int32))


def close_episode(row, store, count, dropped, b, min_amplitude):
    if row[EP_OPEN] == 0:
        return
    row[EP_OPEN] = 0.0
    if not abs(row[EP_D_END] - row[EP_D_START]) >= min_amplitude:
        return
    row[EP_COUNT] = row[EP_COUNT] + 1.0
    if count[b] < store.shape[1]:
        store[b, count[b]] = (row[EP_PHASE], row[EP_T_START], row[EP_T_END], row[EP_D_START], row[EP_D_END], row[EP_PEAK], row[EP_SAMPLES], row[EP_LF])
        count[b] += 1
    else:
        dropped[b] += 1


def run(spec, left, right, state, table, light, store, count, dropped, eye_valid=None, frame_time=None, lengths=None, reset=None, flush=None,
        luminance=None, baseline_mark=None):
    size = np.stack([np.asarray(left, dtype=np.float32), np.asarray(right, dtype=np.float32)])
    B, T = size.shape[1:]
    nan32 = np.float32(np.nan)
    out = {k: np.full((B, T), nan32, dtype=np.float32) for k in KEYS[:5]}
    out.update(valid=np.zeros((B, T), np.uint8), eye_used=np.zeros((B, T, 2), np.uint8), eye_reason=np.zeros((B, T, 2), np.uint8),
               event=np.zeros((B, T), np.uint8))
    fps = None if spec.fps is None else F64(spec.fps)
    min_mm, max_mm, max_speed, max_gap = F64(spec.min_mm), F64(spec.max_mm), F64(spec.max_speed_mm_s), F64(spec.max_gap_s)
    rate, cutoff, light_tau = F64(spec.offset_rate), F64(spec.cutoff_hz), F64(spec.light_tau_s)
    base_tau = F64(0.0 if spec.baseline_tau_s is None else spec.baseline_tau_s)
    dilate, constrict, min_amp = F64(spec.dilate_mm_s), F64(spec.constrict_mm_s), F64(spec.min_amplitude_mm)
    one, half = F64(1.0), F64(0.5)
    with np.errstate(all='ignore'):
        for b in range(B):
            row, tab, lt = state[b], table[b], light[b]
            if reset is not None and reset[b] != 0:
                close_episode(row, store, count, dropped, b, min_amp)
                keep = row[EP_COUNT]
                row[:] = 0.0
                row[EP_COUNT] = keep
            n_frames = T if lengths is None else min(max(int(lengths[b]), 0), T)
            ticks0 = row[TICKS]
            for f in range(n_frames):
                # 1 time
                tt = F64(frame_time[b, f]) if frame_time is not None else (ticks0 + F64(f)) / fps
                if not np.isfinite(tt) or (row[HAS_PREV] != 0 and not tt > row[T_PREV]):
                    continue                                     # not timed: nothing moves
                mark = baseline_mark is not None and baseline_mark[b, f] != 0
                # 2 the luminance's own low pass
                if luminance is not None:
                    lum = F64(np.float32(luminance[b, f]))
                    if np.isfinite(lum) and (row[HAS_LUM] == 0 or tt > row[T_LUM]):
                        dtl = tt - row[T_LUM]
                        if row[HAS_LUM] == 0 or dtl > max_gap:
                            row[LF] = lum
                        else:
                            al = one / (one + light_tau / dtl)
                            row[LF] = al * lum + (one - al) * row[LF]
                        row[HAS_LUM], row[T_LUM] = 1.0, tt
                # 3 acceptance
                acc, val = [False, False], [F64(0.0), F64(0.0)]
                for e in range(2):
                    se = HAS_L + 3 * e
                    why = 0
                    if eye_valid is not None and eye_valid[b, f, e] == 0:
                        why = WITHHELD
                    else:
                        v = F64(size[e, b, f])
                        if not np.isfinite(v):
                            why = NOT_FINITE
                        elif not (min_mm <= v and v <= max_mm):
                            why = RANGE
                        elif row[se] != 0 and tt - row[se + 1] <= max_gap:
                            if not abs(v - row[se + 2]) / (tt - row[se + 1]) <= max_speed:
                                why = SPEED
                        if why == 0:
                            acc[e], val[e] = True, v
                    if why in (NOT_FINITE, RANGE, SPEED):
                        tab[REJ + 3 * e + (NOT_FINITE, RANGE, SPEED).index(why)] += 1.0
                    out['eye_reason'][b, f, e] = why
                if acc[0] or acc[1]:
                    # 4 fusion
                    l, r = val
                    if acc[0] and acc[1]:
                        diff = l - r
                        row[OFF] = row[OFF] + rate * (diff - row[OFF]) if row[HAS_OFF] != 0 else diff
                        row[HAS_OFF] = 1.0
                        d = half * (l + r)
                        tab[BOTH] += 1.0
                    elif acc[0]:
                        d = l - half * row[OFF] if row[HAS_OFF] != 0 else l
                        tab[LEFT] += 1.0
                    else:
                        d = r + half * row[OFF] if row[HAS_OFF] != 0 else r
                        tab[RIGHT] += 1.0
                    # 5 filter
                    dt = tt - row[T_PREV]
                    restart = row[HAS_PREV] == 0 or dt > max_gap
                    idx = ticks0 + F64(f)
                    vel = F64(np.nan)
                    if restart:
                        df = d
                        close_episode(row, store, count, dropped, b, min_amp)
                    else:
                        a = one / (one + (one / (TWO_PI * cutoff)) / dt)
                        df = a * d + (one - a) * row[DF]
                        vel = (df - row[DF]) / dt
                        tab[COVERED] = tab[COVERED] + dt
                        if idx - row[LAST_IDX] != 1.0:
                            tab[LOST] = tab[LOST] + dt
                    # 6 light
                    dc = df
                    lit = luminance is not None and row[HAS_LUM] != 0
                    if lit:
                        if tab[N] == 0:
                            tab[X0], tab[Y0] = row[LF], df
                        dx, dy = row[LF] - tab[X0], df - tab[Y0]
                        tab[N] += 1.0
                        tab[SX] = tab[SX] + dx
                        tab[SY] = tab[SY] + dy
                        tab[SXX] = tab[SXX] + dx * dx
                        tab[SXY] = tab[SXY] + dx * dy
                        tab[SYY] = tab[SYY] + dy * dy
                        if lt[0] != 0:
                            dc = df - lt[1] * (row[LF] - lt[2])
                    # 7 baseline
                    if baseline_mark is not None:
                        if mark:
                            if row[PREV_MARK] == 0:
                                row[B_D0], row[B_N], row[B_SUM] = dc, 0.0, 0.0
                            row[B_N] = row[B_N] + 1.0
                            row[B_SUM] = row[B_SUM] + (dc - row[B_D0])
                            row[BASE] = row[B_D0] + row[B_SUM] / row[B_N]
                            row[HAS_BASE] = 1.0
                    elif base_tau > 0:
                        if row[HAS_BASE] == 0 or row[HAS_PREV] == 0:
                            row[BASE] = dc
                        else:
                            row[BASE] = row[BASE] + (one / (one + base_tau / dt)) * (dc - row[BASE])
                        row[HAS_BASE] = 1.0
                    if (baseline_mark is not None or base_tau > 0) and row[HAS_BASE] != 0:
                        out['change_mm'][b, f] = np.float32(dc - row[BASE])
                        out['change_pct'][b, f] = np.float32(F64(100.0) * (dc - row[BASE]) / row[BASE])
                    # 8 episodes
                    phase = 1 if vel > dilate else (-1 if vel < -constrict else 0)
                    if row[EP_OPEN] != 0 and F64(phase) != row[EP_PHASE]:
                        close_episode(row, store, count, dropped, b, min_amp)
                    if phase != 0:
                        if row[EP_OPEN] == 0:
                            row[EP_OPEN], row[EP_PHASE], row[EP_T_START], row[EP_D_START] = 1.0, F64(phase), row[T_PREV], row[DF]
                            row[EP_PEAK], row[EP_SAMPLES], row[EP_LF] = 0.0, 0.0, (row[LF] if lit else 0.0)
                        row[EP_T_END], row[EP_D_END] = tt, df
                        if abs(vel) > row[EP_PEAK]:
                            row[EP_PEAK] = abs(vel)
                        row[EP_SAMPLES] = row[EP_SAMPLES] + 1.0
                    # 9 table and hand-over
                    if tab[BOTH] + tab[LEFT] + tab[RIGHT] == 1.0:
                        tab[D0] = tab[MIN] = tab[MAX] = dc
                    dd = dc - tab[D0]
                    tab[S1] = tab[S1] + dd
                    tab[S2] = tab[S2] + dd * dd
                    if dc < tab[MIN]:
                        tab[MIN] = dc
                    if dc > tab[MAX]:
                        tab[MAX] = dc
                    if acc[0]:
                        row[HAS_L], row[T_L], row[V_L] = 1.0, tt, l
                    if acc[1]:
                        row[HAS_R], row[T_R], row[V_R] = 1.0, tt, r
                    row[HAS_PREV], row[T_PREV], row[DF], row[LAST_IDX] = 1.0, tt, df, idx
                    out['mm'][b, f], out['raw_mm'][b, f], out['velocity'][b, f] = np.float32(dc), np.float32(d), np.float32(vel)
                    out['valid'][b, f] = 1
                    out['eye_used'][b, f] = acc
                    out['event'][b, f] = 1 if phase == 1 else (2 if phase == -1 else 0)
                if baseline_mark is not None:
                    row[PREV_MARK] = 1.0 if mark else 0.0
            row[TICKS] = ticks0 + F64(n_frames)
            if flush is not None and flush[b] != 0:
                close_episode(row, store, count, dropped, b, min_amp)
    return out
