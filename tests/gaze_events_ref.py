"""The gaze filter and the fixation / saccade events of include/eve_hip.h (eve_gaze_events) in numpy float64: the contract the HIP
kernel follows.  Every operation is one IEEE double operation rounded on its own, in the order written here; the kernel differs
only where libm and the device differ (atan2; sqrt is correctly rounded on both).  Per stream the frames are walked in time order
with a carried state row of 32 doubles (STATE below), so any split of a clip into chunks gives the bits of one pass.

    out = run(spec, pog, o, inv_cam, ppm, state, store, count, dropped, frame_time=, valid=, lengths=, reset=, flush=, log=)

spec: anything with the attributes of eve_amd.GazeEventSpec (Spec below is a plain stand-in).  pog [B, T, 2], o [B, T, 3], inv_cam
[B, T, 4, 4], ppm [B, T, 2] float32; state float64 [B, 32], store float64 [B, F, 8], count and dropped int32 [B]: UPDATED IN PLACE."""
import numpy as np

STATE_DOUBLES = 32
# the state row
TICKS, HAS_PREV, T_PREV, XR_PREV, YR_PREV, XH, YH, DXH, DYH, V0, V1, V2 = range(12)
FIX_OPEN, FIX_ID, NEXT_ID, X0, Y0, FIX_N, SDX, SDY, SD2, T_START, T_LAST = range(12, 23)
TWO_PI = np.float64(6.283185307179586)
RAD2DEG = np.float64(57.29577951308232)
F64 = np.float64


class Spec(object):
    def __init__(self, fps=None, min_cutoff_hz=1.0, beta=0.007, d_cutoff_hz=1.0, velocity_from='filtered', saccade_deg_s=30.0,
                 min_fixation_s=0.06, max_gap_s=0.075):
        self.fps, self.min_cutoff_hz, self.beta, self.d_cutoff_hz = fps, min_cutoff_hz, beta, d_cutoff_hz
        self.velocity_from, self.saccade_deg_s, self.min_fixation_s, self.max_gap_s = velocity_from, saccade_deg_s, min_fixation_s, max_gap_s


def fresh(B, capacity):
    """-> (state, store, count, dropped) of B streams that have seen nothing."""
    return (np.zeros((B, STATE_DOUBLES)), np.zeros((B, capacity, 8)), np.zeros(B, dtype=np.int32), np.zeros(B, dtype=np.int32))


def alpha(fc, dt):
    return F64(1.0) / (F64(1.0) + (F64(1.0) / (TWO_PI * fc)) / dt)


def open_fixation(row):
    """The open fixation of a state row as a store row (id, t_start, t_last, n, cx, cy, rms_px, 0.0), or None."""
    if row[FIX_OPEN] == 0:
        return None
    n = row[FIX_N]
    mx, my = row[SDX] / n, row[SDY] / n
    var = row[SD2] / n - (mx * mx + my * my)
    rms = np.sqrt(var) if var > 0 else F64(0.0)
    return np.array([row[FIX_ID], row[T_START], row[T_LAST], n, row[X0] + mx, row[Y0] + my, rms, 0.0])


def close_fixation(row, min_fixation_s, store, count, dropped, b, log=None):
    done = open_fixation(row)
    row[FIX_OPEN] = 0.0
    if done is not None and log is not None:
        log['closings'].append(float(row[T_LAST] - row[T_START]))
    if done is None or not (row[T_LAST] - row[T_START] >= min_fixation_s):
        return
    if count[b] < store.shape[1]:
        store[b, count[b]] = done
        count[b] += 1
    else:
        dropped[b] += 1


def run(spec, pog, o, inv_cam, ppm, state, store, count, dropped, frame_time=None, valid=None, lengths=None, reset=None, flush=None, log=None):
    pog, o, inv_cam, ppm = (np.asarray(a, dtype=np.float32) for a in (pog, o, inv_cam, ppm))
    B, T = pog.shape[:2]
    nan32 = np.float32(np.nan)
    out = {'PoG_px_filtered': pog.copy(), 'gaze_velocity': np.full((B, T), nan32, dtype=np.float32),
           'gaze_event': np.zeros((B, T), dtype=np.uint8), 'fixation_id': np.full((B, T), -1, dtype=np.int32),
           'fixation_px': np.zeros((B, T, 2), dtype=np.float32), 'fixation_ms': np.zeros((B, T), dtype=np.float32),
           'fixating': np.zeros((B, T), dtype=np.uint8)}
    fps = None if spec.fps is None else F64(spec.fps)
    min_cutoff, beta, d_cutoff = F64(spec.min_cutoff_hz), F64(spec.beta), F64(spec.d_cutoff_hz)
    thr, min_fix, max_gap = F64(spec.saccade_deg_s), F64(spec.min_fixation_s), F64(spec.max_gap_s)
    raw = spec.velocity_from == 'raw'
    with np.errstate(all='ignore'):
        for b in range(B):
            row = state[b]
            if reset is not None and reset[b] != 0:
                close_fixation(row, min_fix, store, count, dropped, b, log)
                keep = row[NEXT_ID]
                row[:] = 0.0
                row[NEXT_ID] = keep
            n_frames = T if lengths is None else min(max(int(lengths[b]), 0), T)
            ticks0 = row[TICKS]
            for t in range(n_frames):
                tt = F64(frame_time[b, t]) if frame_time is not None else (ticks0 + F64(t)) / fps
                x, y = F64(pog[b, t, 0]), F64(pog[b, t, 1])
                oo, Tm, sx, sy = o[b, t].astype(F64), inv_cam[b, t].astype(F64), F64(ppm[b, t, 0]), F64(ppm[b, t, 1])
                e = [((Tm[i, 0] * oo[0] + Tm[i, 1] * oo[1]) + Tm[i, 2] * oo[2]) + Tm[i, 3] for i in range(3)]
                ok = (valid is None or valid[b, t] != 0) and np.isfinite(tt) and np.isfinite([x, y, sx, sy]).all() and \
                    np.isfinite(oo).all() and np.isfinite(Tm).all() and e[2] != 0
                if not ok or (row[HAS_PREV] != 0 and not tt > row[T_PREV]):
                    continue                                     # not a sample: nothing but ticks moves
                restart = row[HAS_PREV] == 0 or tt - row[T_PREV] > max_gap
                dt = tt - row[T_PREV]
                if log is not None and row[HAS_PREV] != 0:
                    log['intervals'].append(float(dt))
                if restart:
                    xh, yh, dxh, dyh = x, y, F64(0.0), F64(0.0)
                else:                                            # the one-euro filter, x and y on their own
                    ad = alpha(d_cutoff, dt)
                    dxh = ad * ((x - row[XR_PREV]) / dt) + (F64(1.0) - ad) * row[DXH]
                    dyh = ad * ((y - row[YR_PREV]) / dt) + (F64(1.0) - ad) * row[DYH]
                    ax, ay = alpha(min_cutoff + beta * np.abs(dxh), dt), alpha(min_cutoff + beta * np.abs(dyh), dt)
                    xh = ax * x + (F64(1.0) - ax) * row[XH]
                    yh = ay * y + (F64(1.0) - ay) * row[YH]
                px, py = (x, y) if raw else (xh, yh)
                v = [px / sx - e[0], py / sy - e[1], -e[2]]
                velocity = F64(np.nan)
                if not restart:
                    p = [row[V0], row[V1], row[V2]]
                    c = [p[1] * v[2] - p[2] * v[1], p[2] * v[0] - p[0] * v[2], p[0] * v[1] - p[1] * v[0]]
                    angle = np.arctan2(np.sqrt((c[0] * c[0] + c[1] * c[1]) + c[2] * c[2]), (p[0] * v[0] + p[1] * v[1]) + p[2] * v[2])
                    velocity = angle * RAD2DEG / dt
                    if log is not None:
                        log['velocities'].append(float(velocity))
                row[HAS_PREV], row[T_PREV], row[XR_PREV], row[YR_PREV] = 1.0, tt, x, y
                row[XH], row[YH], row[DXH], row[DYH] = xh, yh, dxh, dyh
                row[V0], row[V1], row[V2] = v
                out['PoG_px_filtered'][b, t] = (np.float32(xh), np.float32(yh))
                out['gaze_velocity'][b, t] = np.float32(velocity)
                if restart:                                      # a gap (or the first sample): no velocity, no label
                    close_fixation(row, min_fix, store, count, dropped, b, log)
                elif velocity > thr:
                    out['gaze_event'][b, t] = 2
                    close_fixation(row, min_fix, store, count, dropped, b, log)
                else:
                    out['gaze_event'][b, t] = 1
                    if row[FIX_OPEN] == 0:
                        row[FIX_OPEN], row[FIX_ID], row[NEXT_ID] = 1.0, row[NEXT_ID], row[NEXT_ID] + 1.0
                        row[X0], row[Y0], row[FIX_N], row[SDX], row[SDY], row[SD2], row[T_START] = x, y, 0.0, 0.0, 0.0, 0.0, tt
                    ddx, ddy = x - row[X0], y - row[Y0]
                    row[FIX_N] += 1.0
                    row[SDX] += ddx
                    row[SDY] += ddy
                    row[SD2] += ddx * ddx + ddy * ddy
                    row[T_LAST] = tt
                    out['fixation_id'][b, t] = int(row[FIX_ID])
                    out['fixation_px'][b, t] = (np.float32(row[X0] + row[SDX] / row[FIX_N]), np.float32(row[Y0] + row[SDY] / row[FIX_N]))
                    out['fixation_ms'][b, t] = np.float32(F64(1000.0) * (tt - row[T_START]))
                    out['fixating'][b, t] = 1 if tt - row[T_START] >= min_fix else 0
            row[TICKS] = ticks0 + F64(n_frames)
            if flush is not None and flush[b] != 0:
                close_fixation(row, min_fix, store, count, dropped, b, log)
    return out


def new_log():
    return {'velocities': [], 'intervals': [], 'closings': []}


def thresholds_clear(spec, log, margin=1e-9):
    """Exact label equality between two implementations is fair only away from the thresholds: True iff, over the runs that wrote
    `log` (run(..., log=new_log())), no velocity is within `margin` (relative) of saccade_deg_s, no interval between a sample and
    the one before it within it of max_gap_s, and no closing fixation's duration within it of min_fixation_s."""
    near = lambda a, thr: bool(len(a)) and bool((np.abs(np.asarray(a, dtype=np.float64) - thr) <= margin * abs(thr)).any())
    vel = np.asarray(log['velocities'], dtype=np.float64)
    return not (near(vel[np.isfinite(vel)], spec.saccade_deg_s) or near(log['intervals'], spec.max_gap_s) or
                near(log['closings'], spec.min_fixation_s))
