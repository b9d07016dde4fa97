"""The numpy contract of the time-decayed gaze history (eve_gaze_history_plan + eve_gaze_history_update, include/eve_hip.h): per
stream the recurrence M_t = decay^(dt_ms) * M_{t-1} + w_t * G_t over a float32 map that is rounded after every frame.  Float64, every
operation rounded on its own, in the order written here; the device equals it bit for bit, exp included, because the contract owns
its exp (gh_exp).  Nothing here depends on how a clip is cut into chunks."""
import math

import numpy as np

LOG2E = 1.4426950408889634
LN2_HI = 6.93147180369123816490e-01
LN2_LO = 1.90821492927058770002e-10
# 1 / j!, j = 0 .. 13, correctly rounded
EXP_COEF = (1.0, 1.0, 0.5, 0.16666666666666666, 0.041666666666666664, 0.008333333333333333, 0.001388888888888889, 0.0001984126984126984,
            2.48015873015873e-05, 2.7557319223985893e-06, 2.755731922398589e-07, 2.505210838544172e-08, 2.08767569878681e-09,
            1.6059043836821613e-10)
EXP_MIN = -104.0                         # below it gh_exp is exactly 0
TINY = 2.0 ** -100                       # a map value below it is stored as 0: no float32 denormal is ever produced
STATE = 8
HAS_PREV, T_PREV, TICKS = 0, 1, 2
SOURCES = ('PoG_px_initial', 'PoG_px_final', 'PoG_px_filtered', 'fixation_px', 'heatmap_final')


def gh_exp(x):
    """exp(x) for x <= 0 by the contract's recipe: k = rint(x * log2 e), r = (x - k * ln2_hi) - k * ln2_lo, the degree-13 Taylor
    polynomial by Horner's rule, ldexp.  x < -104 gives 0."""
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(invalid='ignore', over='ignore'):
        xc = np.where(x < EXP_MIN, EXP_MIN, x)
        k = np.rint(xc * LOG2E)
        r = (xc - k * LN2_HI) - k * LN2_LO
        p = np.full_like(r, EXP_COEF[13])
        for c in EXP_COEF[12::-1]:
            p = p * r + c
        out = np.ldexp(p, np.where(np.isfinite(k), k, 0.0).astype(np.int64))
        return np.where(x < EXP_MIN, 0.0, out)


def fresh(B, MH, MW):
    """-> (state float64 [B, 8], maps float32 [B, MH, MW]), zero."""
    return np.zeros((B, STATE), dtype=np.float64), np.zeros((B, MH, MW), dtype=np.float32)


def params(size, sigma, decay_per_ms=1.0, weight='frame', max_gap_s=0.075, fps=None, floor=0.0, normalize=False):
    """The launch's scalars from a spec's numbers (what the host computes in double)."""
    return {'size': (int(size[0]), int(size[1])), 'alpha': -0.5 / (float(sigma) * float(sigma)), 'ln_decay': math.log(float(decay_per_ms)),
            'seconds': weight == 'seconds', 'max_gap_s': float(max_gap_s), 'fps': None if fps is None else float(fps), 'floor': float(floor),
            'gain': 1.0 / (2.0 * math.pi * float(sigma) * float(sigma)) if normalize else 1.0}


def spec_params(spec, config=None):
    """params() of an eve_amd.GazeHistorySpec, the config's defaults filled in as EVEStream.step does."""
    size, sigma, decay = spec.resolved(config)
    return params(size, sigma, decay, spec.weight, spec.max_gap_s, spec.fps, spec.floor, spec.normalize)


def run(P, screen_size, state, maps, T, pog=None, heat=None, frame_time=None, valid=None, valid_key=None, lengths=None, reset=None,
        per_frame=False):
    """One chunk of B streams x T frames.  state [B, 8] float64 and maps [B, MH, MW] float32 are UPDATED IN PLACE.  pog [B, T, 2]
    float32 (screen pixels) or heat [B, T, MH, MW] float32 (the heat-map source); frame_time [B, T] float64 or None (then ticks / fps);
    valid, valid_key [B, T] bool / uint8 or None; lengths, reset [B] ints or None.  -> float32 [B, T, MH, MW] where per_frame, else None."""
    B, MH, MW = maps.shape
    assert P['size'] == (MW, MH) and state.shape == (B, STATE) and maps.dtype == np.float32 and state.dtype == np.float64
    assert (pog is None) != (heat is None) or T == 0
    frame_time, valid, valid_key = (None if a is None else np.asarray(a) for a in (frame_time, valid, valid_key))
    frames = np.zeros((B, T, MH, MW), dtype=np.float32) if per_frame else None
    sx, sy = float(MW) / float(screen_size[0]), float(MH) / float(screen_size[1])
    xs, ys = np.arange(MW, dtype=np.float64), np.arange(MH, dtype=np.float64)
    fps, floor, alpha = P['fps'], np.float64(P['floor']), np.float64(P['alpha'])
    with np.errstate(all='ignore'):
        for b in range(B):
            st, m = state[b], maps[b]
            if reset is not None and reset[b] != 0:
                st[:] = 0.0
                m[:] = 0.0
            n = T if lengths is None else min(max(int(lengths[b]), 0), T)
            for t in range(n):
                tt = np.float64(frame_time[b, t]) if frame_time is not None else np.float64(st[TICKS]) / np.float64(fps)
                st[TICKS] += 1.0
                has_prev = st[HAS_PREV] != 0.0
                if not np.isfinite(tt) or (has_prev and tt < st[T_PREV]):
                    if per_frame:
                        frames[b, t] = m
                    continue
                delta = tt - st[T_PREV] if has_prev else np.float64(0.0)
                d = np.float64(gh_exp((delta * 1000.0) * P['ln_decay']))
                usable = (valid is None or valid[b, t] != 0) and (valid_key is None or valid_key[b, t] != 0)
                if heat is None:
                    px, py = np.float64(pog[b, t, 0]), np.float64(pog[b, t, 1])
                    usable = usable and bool(np.isfinite(px)) and bool(np.isfinite(py))
                if not P['seconds']:
                    base = np.float64(1.0)
                elif has_prev:
                    base = min(delta, np.float64(P['max_gap_s']))
                else:
                    base = np.float64(1.0) / np.float64(fps) if fps is not None else np.float64(0.0)
                w = np.float64(P['gain']) * base
                st[HAS_PREV], st[T_PREV] = 1.0, tt
                v = m.astype(np.float64) * d
                if usable:
                    if heat is None:
                        cx, cy = sx * px, sy * py
                        ex = gh_exp(alpha * ((xs - cx) * (xs - cx)))
                        ey = gh_exp(alpha * ((ys - cy) * (ys - cy)))
                        v = v + w * (ex[None, :] * ey[:, None] + floor)
                    else:
                        v = v + w * heat[b, t].astype(np.float64)
                m[:] = np.where(np.abs(v) < TINY, 0.0, v).astype(np.float32)
                if per_frame:
                    frames[b, t] = m
    return frames
