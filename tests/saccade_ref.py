"""The saccade stage of include/eve_hip.h (eve_gaze_events_ex, eve_gaze_saccades) in numpy float64: the contract the HIP kernels follow.

    ex = events_ex(spec, pog, o, inv_cam, ppm, state, store, count, dropped, frame_time=, valid=, lengths=, reset=, flush=, log=)

is gaze_events_ref.run's result plus `sample` uint8 [B, T], `sample_time` float64 [B, T] and `gaze_vector` float64 [B, T, 3].  It does
not restate the events' arithmetic: it walks gaze_events_ref.run one frame at a time -- any split of a clip gives the bits of one pass,
which the events' own suite pins -- and reads the three off the state row after each frame.

    out = run(saccade_spec, sample, sample_time, gaze_vector, point, event, velocity, fixation_id, state, table, store, count, dropped,
              lengths=, reset=, log=)

are the saccade rules: every operation is one IEEE double operation rounded on its own, in the order written here; the kernel differs
only where libm and the device differ (atan2; sqrt is correctly rounded on both).  state float64 [B, 32] (STATE below), table float64
[B, 16], store float64 [B, S, 16], count and dropped int32 [B]: UPDATED IN PLACE.  -> {'saccade_id': int32 [B, T], 'saccade_ms': float32
[B, T]}."""
import numpy as np

import gaze_events_ref as events

STATE_DOUBLES = 32
ROW = 16
# the state row
HAS_PREV, T_PREV, PV0, PV1, PV2, PX, PY, P_EVENT, P_FIX, OPEN, ID, NEXT_ID, T_ONSET, OV0, OV1, OV2, X0, Y0, N, PEAK, MISSING, PREV_FIX = range(22)
# the table row
ACCEPTED, SUM_A, SUM_AA, SUM_P, SUM_AP, SUM_D, SUM_AD, MAX_A, MAX_P, ABORTED, SMALL, SHORT, LONG, INTERRUPTED = range(14)
# the store row
R_ID, R_T0, R_T1, R_N, R_X0, R_Y0, R_X1, R_Y1, R_AMP, R_PEAK, R_MEAN, R_PREV_FIX, R_NEXT_FIX, R_MISSING = range(14)
TRANSCENDENTAL_ROW = (R_AMP, R_MEAN)                     # the store columns behind an atan2; every other one is exact
TRANSCENDENTAL_TABLE = (SUM_A, SUM_AA, SUM_AP, SUM_AD, MAX_A)
PEAK_ROW = (R_PEAK,)                                     # ... and those that hold a float32 velocity of the events launch
PEAK_TABLE = (SUM_P, SUM_AP, MAX_P)
RAD2DEG = np.float64(57.29577951308232)
F64 = np.float64


class Spec(object):
    """A plain stand-in with the attributes of eve_amd.SaccadeSpec."""

    def __init__(self, min_amplitude_deg=0.5, min_duration_s=0.0, max_duration_s=0.2, max_missing=0):
        self.min_amplitude_deg, self.min_duration_s, self.max_duration_s, self.max_missing = min_amplitude_deg, min_duration_s, max_duration_s, max_missing


def fresh(B, capacity):
    """-> (state, table, store, count, dropped) of B streams that have seen nothing."""
    return (np.zeros((B, STATE_DOUBLES)), np.zeros((B, ROW)), np.zeros((B, capacity, ROW)), np.zeros(B, dtype=np.int32),
            np.zeros(B, dtype=np.int32))


def events_ex(spec, pog, o, inv_cam, ppm, state, store, count, dropped, frame_time=None, valid=None, lengths=None, reset=None, flush=None,
              log=None):
    pog = np.asarray(pog, dtype=np.float32)
    B, T = pog.shape[:2]
    out = None
    sample, sample_time, vector = np.zeros((B, T), dtype=np.uint8), np.zeros((B, T)), np.zeros((B, T, 3))
    n_frames = np.full(B, T) if lengths is None else np.clip(np.asarray(lengths), 0, T)
    if reset is not None:                                # the launch with no frames: the reset alone
        events.run(spec, pog[:, :0], o[:, :0], inv_cam[:, :0], ppm[:, :0], state, store, count, dropped, reset=reset, log=log)
    for t in range(T):
        before = state.copy()
        cut = lambda a: None if a is None else np.asarray(a)[:, t:t + 1]
        one = events.run(spec, pog[:, t:t + 1], cut(o), cut(inv_cam), cut(ppm), state, store, count, dropped, frame_time=cut(frame_time),
                         valid=cut(valid), lengths=(n_frames > t).astype(np.int32), log=log)
        if out is None:
            out = {k: np.zeros((B, T) + v.shape[2:], dtype=v.dtype) for k, v in one.items()}
        for k, v in one.items():
            out[k][:, t] = v[:, 0]
        for b in range(B):
            if state[b, events.T_PREV] != before[b, events.T_PREV] or state[b, events.HAS_PREV] != before[b, events.HAS_PREV]:
                sample[b, t] = 2 if one['gaze_event'][b, 0] != 0 else 1
                sample_time[b, t] = state[b, events.T_PREV]
                vector[b, t] = state[b, events.V0:events.V2 + 1]
    if flush is not None:
        events.run(spec, pog[:, :0], o[:, :0], inv_cam[:, :0], ppm[:, :0], state, store, count, dropped, flush=flush, log=log)
    if out is None:
        out = {}
    out.update(sample=sample, sample_time=sample_time, gaze_vector=vector)
    return out


def point_of(spec, pog, ex):
    """The point the velocity is from: the source with velocity_from='raw', else the filtered one."""
    return np.asarray(pog, dtype=np.float32) if spec.velocity_from == 'raw' else ex['PoG_px_filtered']


def amplitude(p, v):
    c = [p[1] * v[2] - p[2] * v[1], p[2] * v[0] - p[0] * v[2], p[0] * v[1] - p[1] * v[0]]
    return np.arctan2(np.sqrt((c[0] * c[0] + c[1] * c[1]) + c[2] * c[2]), (p[0] * v[0] + p[1] * v[1]) + p[2] * v[2]) * RAD2DEG


def abort(row, tab):
    if row[OPEN] != 0:
        row[OPEN] = 0.0
        tab[ABORTED] += 1.0


def run(spec, sample, sample_time, gaze_vector, point, event, velocity, fixation_id, state, table, store, count, dropped, lengths=None,
        reset=None, log=None):
    B = state.shape[0]
    T = 0 if sample is None else np.asarray(sample).shape[1]
    out = {'saccade_id': np.full((B, T), -1, dtype=np.int32), 'saccade_ms': np.zeros((B, T), dtype=np.float32)}
    min_amp, min_dur, max_dur = F64(spec.min_amplitude_deg), F64(spec.min_duration_s), F64(spec.max_duration_s)
    max_missing = F64(spec.max_missing)
    with np.errstate(all='ignore'):
        for b in range(B):
            row, tab = state[b], table[b]
            if reset is not None and reset[b] != 0:
                abort(row, tab)
                keep = row[NEXT_ID]
                row[:] = 0.0
                row[NEXT_ID] = keep
            n_frames = T if lengths is None else min(max(int(lengths[b]), 0), T)
            for t in range(n_frames):
                fl = int(sample[b, t])
                if fl == 0:
                    if row[OPEN] != 0:
                        row[MISSING] += 1.0
                    continue
                tt = F64(sample_time[b, t])
                ev = int(event[b, t]) if fl == 2 else 0
                if fl != 2 or ev not in (1, 2):
                    abort(row, tab)
                elif ev == 2:
                    if row[OPEN] == 0 and row[HAS_PREV] != 0 and row[P_EVENT] != 2:
                        row[OPEN], row[ID], row[NEXT_ID] = 1.0, row[NEXT_ID], row[NEXT_ID] + 1.0
                        row[T_ONSET] = row[T_PREV]
                        row[OV0:OV2 + 1] = row[PV0:PV2 + 1]
                        row[X0], row[Y0] = row[PX], row[PY]
                        row[N], row[PEAK], row[MISSING] = 0.0, 0.0, 0.0
                        row[PREV_FIX] = row[P_FIX] if row[P_EVENT] == 1 else -1.0
                    if row[OPEN] != 0:
                        row[N] += 1.0
                        vel = F64(velocity[b, t])
                        if vel > row[PEAK]:
                            row[PEAK] = vel
                        out['saccade_id'][b, t] = int(row[ID])
                        out['saccade_ms'][b, t] = np.float32(F64(1000.0) * (tt - row[T_ONSET]))
                elif row[OPEN] != 0:                             # a fixation frame: the saccade lands at the previous sample
                    row[OPEN] = 0.0
                    amp = amplitude(row[OV0:OV2 + 1].copy(), row[PV0:PV2 + 1].copy())
                    dur = row[T_PREV] - row[T_ONSET]
                    peak, missing = row[PEAK], row[MISSING]
                    if log is not None:
                        log['amplitudes'].append(float(amp))
                        log['durations'].append(float(dur))
                    if missing > max_missing:
                        tab[INTERRUPTED] += 1.0
                    elif dur > max_dur:
                        tab[LONG] += 1.0
                    elif dur < min_dur:
                        tab[SHORT] += 1.0
                    elif not amp >= min_amp:
                        tab[SMALL] += 1.0
                    else:
                        tab[ACCEPTED] += 1.0
                        tab[SUM_A] += amp
                        tab[SUM_AA] += amp * amp
                        tab[SUM_P] += peak
                        tab[SUM_AP] += amp * peak
                        tab[SUM_D] += dur
                        tab[SUM_AD] += amp * dur
                        if amp > tab[MAX_A]:
                            tab[MAX_A] = amp
                        if peak > tab[MAX_P]:
                            tab[MAX_P] = peak
                        if count[b] < store.shape[1]:
                            store[b, count[b]] = [row[ID], row[T_ONSET], row[T_PREV], row[N], row[X0], row[Y0], row[PX], row[PY], amp, peak,
                                                  amp / dur, row[PREV_FIX], F64(fixation_id[b, t]), missing, 0.0, 0.0]
                            count[b] += 1
                        else:
                            dropped[b] += 1
                row[HAS_PREV], row[T_PREV] = 1.0, tt
                row[PV0:PV2 + 1] = gaze_vector[b, t]
                row[PX], row[PY] = F64(point[b, t, 0]), F64(point[b, t, 1])
                row[P_EVENT], row[P_FIX] = F64(ev), F64(fixation_id[b, t])
    return out


def new_log():
    return {'amplitudes': [], 'durations': []}


def thresholds_clear(spec, log, margin=1e-9):
    """Exact equality of the verdicts between two implementations is fair only away from the thresholds: True iff, over the runs that
    wrote `log` (run(..., log=new_log())), no closing saccade's amplitude is within `margin` (relative) of min_amplitude_deg and no
    duration within it of min_duration_s or max_duration_s."""
    near = lambda a, thr: bool(len(a)) and bool((np.abs(np.asarray(a, dtype=np.float64) - thr) <= margin * abs(thr)).any())
    return not (near(log['amplitudes'], spec.min_amplitude_deg) or near(log['durations'], spec.min_duration_s) or
                near(log['durations'], spec.max_duration_s))
