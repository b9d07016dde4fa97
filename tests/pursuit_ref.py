"""The smooth-pursuit stage of include/eve_hip.h (eve_gaze_pursuits) in numpy float64: the contract the HIP kernel follows.

    out = run(pursuit_spec, sample, sample_time, gaze_vector, point, event, velocity, fixation_id, state, table, store, count, dropped,
              target=, lengths=, reset=, log=)

The inputs are those of saccade_ref.run (saccade_ref.events_ex makes them) plus target float32 [B, T, 2] or None.  Every operation is one
IEEE double operation rounded on its own, in the order written here; the kernel differs only where libm and the device differ (atan2;
sqrt is correctly rounded on both).  state float64 [B, 320] (the scalars below, then 32 ring entries of 9 doubles), table float64
[B, 16], store float64 [B, S, 20], count and dropped int32 [B]: UPDATED IN PLACE.  -> {'gaze_class': uint8 [B, T], 'pursuit_id': int32
[B, T], 'pursuit_ms', 'gaze_velocity_windowed', 'gaze_straightness', 'pursuit_gain': float32 [B, T]}."""
import numpy as np

SCALARS = 32
RING = 32
ENTRY = 9
STATE_DOUBLES = SCALARS + RING * ENTRY
TABLE_ROW = 16
ROW = 20
# the state row's scalars
(RING_N, SEEN_SACCADE, T_SACCADE, OPEN, ID, NEXT_ID, T_ONSET, OV0, OV1, OV2, X0, Y0, CUM_ONSET, N, PEAK, MISSING, FIX, T_LAST, LV0, LV1, LV2,
 X1, Y1, CUM_LAST, GAIN_SUM, GAIN_N, ERR_SUM, HAS_END, T_END) = range(29)
# a ring entry
E_T, E_V0, E_V1, E_V2, E_CUM, E_X, E_Y, E_TX, E_TY = range(ENTRY)
# the table row
ACCEPTED, SUM_DUR, SUM_AMP, SUM_PATH, SUM_MEAN_V, MAX_PEAK, SUM_GAIN, TAB_GAIN_N, ABORTED, SMALL, SHORT, INTERRUPTED = range(12)
# the store row
(R_ID, R_T0, R_T1, R_N, R_X0, R_Y0, R_X1, R_Y1, R_AMP, R_DIR, R_MEAN, R_PEAK, R_PATH, R_FIX, R_MISSING, R_GAIN_N, R_GAIN, R_ERR) = range(18)
TRANSCENDENTAL_ROW = (R_AMP, R_DIR, R_MEAN, R_PEAK, R_PATH)      # the store columns behind an atan2 or a float32 velocity of the events launch
TRANSCENDENTAL_TABLE = (SUM_AMP, SUM_PATH, SUM_MEAN_V, MAX_PEAK)
KEYS = ('gaze_class', 'pursuit_id', 'pursuit_ms', 'gaze_velocity_windowed', 'gaze_straightness', 'pursuit_gain')
RAD2DEG = np.float64(57.29577951308232)
F64 = np.float64
NAN = np.float64('nan')


class Spec(object):
    """A plain stand-in with the attributes of eve_amd.PursuitSpec."""

    def __init__(self, window_s=0.2, min_window_s=0.1, pursuit_deg_s=3.0, min_straightness=0.7, settle_s=0.08, min_duration_s=0.15,
                 min_amplitude_deg=1.0, max_missing=3):
        self.window_s, self.min_window_s, self.pursuit_deg_s, self.min_straightness = window_s, min_window_s, pursuit_deg_s, min_straightness
        self.settle_s, self.min_duration_s, self.min_amplitude_deg, self.max_missing = settle_s, min_duration_s, min_amplitude_deg, max_missing


def fresh(B, capacity):
    """-> (state, table, store, count, dropped) of B streams that have seen nothing."""
    return (np.zeros((B, STATE_DOUBLES)), np.zeros((B, TABLE_ROW)), np.zeros((B, capacity, ROW)), np.zeros(B, dtype=np.int32),
            np.zeros(B, dtype=np.int32))


def angle(p, v):
    """The events stage's expression, in degrees."""
    c = [p[1] * v[2] - p[2] * v[1], p[2] * v[0] - p[0] * v[2], p[0] * v[1] - p[1] * v[0]]
    return np.arctan2(np.sqrt((c[0] * c[0] + c[1] * c[1]) + c[2] * c[2]), (p[0] * v[0] + p[1] * v[1]) + p[2] * v[2]) * RAD2DEG


def abort(row, tab):
    if row[OPEN] != 0:
        row[OPEN] = 0.0
        tab[ABORTED] += 1.0


def close(spec, row, tab, store, count, dropped, b, log):
    """The open episode of `row` closes at its last sample: judged, tallied, stored."""
    row[OPEN] = 0.0
    row[HAS_END], row[T_END] = 1.0, row[T_LAST]
    dur = row[T_LAST] - row[T_ONSET]
    amp = angle(row[OV0:OV2 + 1].copy(), row[LV0:LV2 + 1].copy())
    direction = np.arctan2(row[Y1] - row[Y0], row[X1] - row[X0]) * RAD2DEG
    path = row[CUM_LAST] - row[CUM_ONSET]
    if log is not None:
        log['amplitudes'].append(float(amp))
    if row[MISSING] > F64(spec.max_missing):
        tab[INTERRUPTED] += 1.0
    elif dur < F64(spec.min_duration_s):
        tab[SHORT] += 1.0
    elif not amp >= F64(spec.min_amplitude_deg):
        tab[SMALL] += 1.0
    else:
        mean_v = amp / dur
        tab[ACCEPTED] += 1.0
        tab[SUM_DUR] += dur
        tab[SUM_AMP] += amp
        tab[SUM_PATH] += path
        tab[SUM_MEAN_V] += mean_v
        if row[PEAK] > tab[MAX_PEAK]:
            tab[MAX_PEAK] = row[PEAK]
        tab[SUM_GAIN] += row[GAIN_SUM]
        tab[TAB_GAIN_N] += row[GAIN_N]
        if count[b] < store.shape[1]:
            some = row[GAIN_N] > 0
            store[b, count[b]] = [row[ID], row[T_ONSET], row[T_LAST], row[N], row[X0], row[Y0], row[X1], row[Y1], amp, direction, mean_v,
                                  row[PEAK], path, row[FIX], row[MISSING], row[GAIN_N], row[GAIN_SUM] / row[GAIN_N] if some else NAN,
                                  row[ERR_SUM] / row[GAIN_N] if some else NAN, 0.0, 0.0]
            count[b] += 1
        else:
            dropped[b] += 1


def run(spec, sample, sample_time, gaze_vector, point, event, velocity, fixation_id, state, table, store, count, dropped, target=None,
        lengths=None, reset=None, log=None):
    B = state.shape[0]
    T = 0 if sample is None else np.asarray(sample).shape[1]
    nan32 = lambda: np.full((B, T), np.nan, dtype=np.float32)
    out = {'gaze_class': np.zeros((B, T), dtype=np.uint8), 'pursuit_id': np.full((B, T), -1, dtype=np.int32),
           'pursuit_ms': np.zeros((B, T), dtype=np.float32), 'gaze_velocity_windowed': nan32(), 'gaze_straightness': nan32(),
           'pursuit_gain': nan32()}
    window, min_window, settle = F64(spec.window_s), F64(spec.min_window_s), F64(spec.settle_s)
    pursuit, straight = F64(spec.pursuit_deg_s), F64(spec.min_straightness)
    with np.errstate(all='ignore'):
        for b in range(B):
            row, tab = state[b], table[b]
            if reset is not None and reset[b] != 0:
                abort(row, tab)
                keep = row[NEXT_ID]
                row[:] = 0.0
                row[NEXT_ID] = keep
            ring = [row[SCALARS + ENTRY * i:SCALARS + ENTRY * (i + 1)].copy() for i in range(int(row[RING_N]))]
            n_frames = T if lengths is None else min(max(int(lengths[b]), 0), T)
            for f in range(n_frames):
                fl = int(sample[b, f])
                if fl == 0:
                    if row[OPEN] != 0:
                        row[MISSING] += 1.0
                    continue
                t = F64(sample_time[b, f])
                v = np.asarray(gaze_vector[b, f], dtype=np.float64)
                x, y = F64(point[b, f, 0]), F64(point[b, f, 1])
                tx, ty = (NAN, NAN) if target is None else (F64(target[b, f, 0]), F64(target[b, f, 1]))
                ev = int(event[b, f]) if fl == 2 else 0
                if fl != 2 or ev not in (1, 2):              # a restart (sample 2 with another label: eve_gaze_events never writes it)
                    abort(row, tab)
                    row[SEEN_SACCADE], row[HAS_END] = 0.0, 0.0
                    ring = [np.array([t, v[0], v[1], v[2], 0.0, x, y, tx, ty])]
                    continue
                if ev == 2:
                    out['gaze_class'][b, f] = 2
                    if row[OPEN] != 0:
                        close(spec, row, tab, store, count, dropped, b, log)
                    ring = []
                    row[HAS_END] = 0.0
                    row[SEEN_SACCADE], row[T_SACCADE] = 1.0, t
                    continue
                out['gaze_class'][b, f] = 1
                if row[SEEN_SACCADE] != 0 and t - row[T_SACCADE] < settle:
                    continue
                cum = ring[-1][E_CUM] + F64(velocity[b, f]) * (t - ring[-1][E_T]) if ring else F64(0.0)
                ring.append(np.array([t, v[0], v[1], v[2], cum, x, y, tx, ty]))
                ring = ring[-RING:]
                i = j = len(ring) - 1
                while j > 0 and t - ring[j - 1][E_T] <= window:
                    j -= 1
                e = ring[j]
                span = t - e[E_T]
                candidate = False
                w = gain = err = NAN
                if not span < min_window:
                    a = angle(e[E_V0:E_V2 + 1], v)
                    w = a / span
                    path = cum - e[E_CUM]
                    s = a / path if path > 0 else F64(0.0)
                    candidate = bool(w >= pursuit and s >= straight)
                    if np.isfinite(tx) and np.isfinite(ty) and np.isfinite(e[E_TX]) and np.isfinite(e[E_TY]):
                        dtx, dty = tx - e[E_TX], ty - e[E_TY]
                        dgx, dgy = x - e[E_X], y - e[E_Y]
                        den = dtx * dtx + dty * dty
                        if den > 0:
                            gain = (dgx * dtx + dgy * dty) / den
                            err = np.sqrt((x - tx) * (x - tx) + (y - ty) * (y - ty))
                    out['gaze_velocity_windowed'][b, f], out['gaze_straightness'][b, f] = np.float32(w), np.float32(s)
                    out['pursuit_gain'][b, f] = np.float32(gain)
                    if log is not None:
                        log['velocities'].append(float(w))
                        log['straightness'].append(float(s))
                if candidate:
                    if row[OPEN] == 0:
                        k = j
                        if row[HAS_END] != 0:                # episodes never overlap: the onset lies after the last closed one's end
                            while k < i and not ring[k][E_T] > row[T_END]:
                                k += 1
                        o = ring[k]
                        row[OPEN], row[ID], row[NEXT_ID] = 1.0, row[NEXT_ID], row[NEXT_ID] + 1.0
                        row[T_ONSET], row[OV0:OV2 + 1], row[X0], row[Y0], row[CUM_ONSET] = o[E_T], o[E_V0:E_V2 + 1], o[E_X], o[E_Y], o[E_CUM]
                        row[N], row[PEAK], row[MISSING], row[GAIN_SUM], row[GAIN_N], row[ERR_SUM] = 0.0, 0.0, 0.0, 0.0, 0.0, 0.0
                        row[FIX] = F64(fixation_id[b, f])
                    row[N] += 1.0
                    if w > row[PEAK]:
                        row[PEAK] = w
                    row[T_LAST], row[LV0:LV2 + 1], row[X1], row[Y1], row[CUM_LAST] = t, v, x, y, cum
                    if not np.isnan(gain):
                        row[GAIN_SUM] += gain
                        row[ERR_SUM] += err
                        row[GAIN_N] += 1.0
                    out['gaze_class'][b, f] = 3
                    out['pursuit_id'][b, f] = int(row[ID])
                    out['pursuit_ms'][b, f] = np.float32(F64(1000.0) * (t - row[T_ONSET]))
                elif row[OPEN] != 0:
                    close(spec, row, tab, store, count, dropped, b, log)
            row[RING_N] = F64(len(ring))
            row[SCALARS:] = 0.0
            for i, e in enumerate(ring):
                row[SCALARS + ENTRY * i:SCALARS + ENTRY * (i + 1)] = e
    return out


def new_log():
    return {'velocities': [], 'straightness': [], 'amplitudes': []}


def thresholds_clear(spec, log, margin=1e-9):
    """Exact equality of the labels and verdicts between two implementations is fair only away from the thresholds that an atan2
    feeds: True iff, over the runs that wrote `log` (run(..., log=new_log())), no frame's windowed velocity is within `margin`
    (relative) of pursuit_deg_s, no frame's straightness within it of min_straightness and no closing's amplitude within it of
    min_amplitude_deg."""
    near = lambda a, thr: bool(len(a)) and bool((np.abs(np.asarray(a, dtype=np.float64) - thr) <= margin * abs(thr)).any())
    return not (near(log['velocities'], spec.pursuit_deg_s) or near(log['straightness'], spec.min_straightness) or
                near(log['amplitudes'], spec.min_amplitude_deg))
