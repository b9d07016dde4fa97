"""The eye gate in numpy: the contract of eve_eye_gate (include/eve_hip.h) restated operation by operation, in float64 with the
header's association, every operation rounded on its own.  The HIP kernel must give these bits.

    state, store, count, dropped = fresh(B, capacity)
    out = run(params, B, T, state, store, count, dropped, pose_valid=..., reproj_rms=..., inliers=..., warp=..., h=..., contours=...,
              lengths=..., reset=..., frame=(IW, IH), patch=(OW, OH))       # state, store, count, dropped UPDATED IN PLACE
    -> {'usable', 'reason', 'blink': uint8 [B, T, 2], 'openness': float32 [B, T, 2]}

params: a dict of the parameter block's fields (params_of(spec) makes one from an eve_amd.EyeGateSpec)."""
import numpy as np

HAS_BASE, BASE, CLOSED, RUN, MIN_OPEN, START, HOLD, TICK = range(8)
R_POSE, R_REPROJ, R_INLIERS, R_COVERAGE, R_HEAD, R_CLOSED, R_HOLD = 1, 2, 4, 8, 16, 32, 64
INF = float('inf')
DEFAULTS = dict(max_reproj_px=INF, min_inliers=0, min_inside=1, pitch_lo=-INF, pitch_hi=INF, yaw_lo=(-INF, -INF), yaw_hi=(INF, INF),
                close_ratio=0.65, open_ratio=0.75, baseline_rate=0.02, baseline_rise=0.5, hold_frames=2, max_closed_frames=90)


def fresh(B, capacity):
    return (np.zeros((B, 2, 8)), np.zeros((B, capacity, 4)), np.zeros(B, dtype=np.int32), np.zeros(B, dtype=np.int32))


def params_of(spec=None, **over):
    """The parameter block of an eve_amd.EyeGateSpec (None: the defaults), with fields overridden by name."""
    p = dict(DEFAULTS)
    if spec is not None:
        if spec.max_reproj_px is not None:
            p['max_reproj_px'] = float(spec.max_reproj_px)
        if spec.min_inliers is not None:
            p['min_inliers'] = int(spec.min_inliers)
        if spec.min_coverage is not None:
            p['min_inside'] = spec.min_inside
        if spec.head_pitch is not None:
            p['pitch_lo'], p['pitch_hi'] = spec.head_pitch
        lo, hi = list(p['yaw_lo']), list(p['yaw_hi'])
        for e, r in enumerate((spec.head_yaw_left, spec.head_yaw_right)):
            if r is not None:
                lo[e], hi[e] = r
        p['yaw_lo'], p['yaw_hi'] = tuple(lo), tuple(hi)
        if spec.blink is not None:
            for name in ('close_ratio', 'open_ratio', 'baseline_rate', 'baseline_rise', 'hold_frames', 'max_closed_frames'):
                p[name] = getattr(spec.blink, name)
    p.update(over)
    return p


def inside_count(m, frame, patch):
    """The lattice points of an OW x OH patch that the warp m (9 values) puts inside the IW x IH frame."""
    IW, IH = frame
    OW, OH = patch
    m = [float(np.float64(v)) for v in np.asarray(m).reshape(9)]
    n = 0
    with np.errstate(all='ignore'):
        for j in range(8):
            for i in range(8):
                ox, oy = np.float64(((2 * i + 1) * OW) >> 4), np.float64(((2 * j + 1) * OH) >> 4)
                X = (np.float64(m[0]) * ox + np.float64(m[1]) * oy) + np.float64(m[2])
                Y = (np.float64(m[3]) * ox + np.float64(m[4]) * oy) + np.float64(m[5])
                Wd = (np.float64(m[6]) * ox + np.float64(m[7]) * oy) + np.float64(m[8])
                u, v = X / Wd, Y / Wd
                n += bool(Wd > 0.0 and u > -1.0 and u < IW and v > -1.0 and v < IH)
    return n


def _dist(a, b):
    dx, dy = a[0] - b[0], a[1] - b[1]
    return np.sqrt(dx * dx + dy * dy)


def eye_aspect_ratio(points):
    """points [6, C] float32 -> (ear float64, known)."""
    p = np.asarray(points).astype(np.float64)
    if not np.isfinite(p[:, :2]).all() or (p.shape[1] == 3 and not (p[:, 2] > 0.0).all()):
        return 0.0, False
    d14 = _dist(p[0], p[3])
    if d14 == 0.0:
        return 0.0, False
    return float((_dist(p[1], p[5]) + _dist(p[2], p[4])) / (2.0 * d14)), True


def run(params, B, T, state, store, count, dropped, pose_valid=None, reproj_rms=None, inliers=None, warp=None, h=None, contours=None,
        lengths=None, reset=None, frame=None, patch=None):
    """pose_valid [B, T, 2], reproj_rms [B, T], inliers [B, T], warp [2, B*T, 9], h [2, B*T, 2], contours [B, T, 2, 6, C], lengths, reset
    [B]: each None or an array."""
    P = params
    capacity = store.shape[1]
    usable, reason = np.zeros((B, T, 2), dtype=np.uint8), np.zeros((B, T, 2), dtype=np.uint8)
    openness, blink = np.full((B, T, 2), np.nan, dtype=np.float32), np.zeros((B, T, 2), dtype=np.uint8)
    for b in range(B):
        if reset is not None and reset[b] != 0:
            state[b] = 0.0
        n = T if lengths is None else min(max(int(lengths[b]), 0), T)
        cnt = min(max(int(count[b]), 0), capacity)
        for f in range(n):
            q = b * T + f
            for e in range(2):
                r = 0
                if pose_valid is not None and pose_valid[b, f, e] == 0:
                    r |= R_POSE
                if reproj_rms is not None and not (np.float64(reproj_rms[b, f]) <= P['max_reproj_px']):
                    r |= R_REPROJ
                if inliers is not None and not (int(inliers[b, f]) >= P['min_inliers']):
                    r |= R_INLIERS
                if warp is not None and inside_count(warp[e, q], frame, patch) < P['min_inside']:
                    r |= R_COVERAGE
                if h is not None:
                    pitch, yaw = np.float64(h[e, q, 0]), np.float64(h[e, q, 1])
                    if not (pitch >= P['pitch_lo'] and pitch <= P['pitch_hi'] and yaw >= P['yaw_lo'][e] and yaw <= P['yaw_hi'][e]):
                        r |= R_HEAD
                opn = np.float64(np.nan)
                if contours is not None:
                    s = state[b, e]
                    ear, known = eye_aspect_ratio(contours[b, f, e])
                    ear = np.float64(ear)
                    tick = s[TICK] + np.float64(f)
                    if known and s[HAS_BASE] == 0.0:
                        s[HAS_BASE], s[BASE] = 1.0, ear
                    with np.errstate(all='ignore'):
                        if known:
                            opn = ear / s[BASE]
                        if s[CLOSED] != 0.0:
                            s[RUN] = s[RUN] + 1.0
                            if known and opn < s[MIN_OPEN]:
                                s[MIN_OPEN] = opn
                            if known and opn > P['open_ratio']:
                                if cnt >= capacity:
                                    dropped[b] += 1
                                else:
                                    store[b, cnt] = (float(e), s[START], tick - 1.0, s[MIN_OPEN])
                                    cnt += 1
                                s[CLOSED], s[RUN], s[HOLD] = 0.0, 0.0, float(P['hold_frames'])
                            elif s[RUN] > float(P['max_closed_frames']):
                                s[HAS_BASE], s[BASE] = (1.0, ear) if known else (0.0, 0.0)
                                s[CLOSED], s[RUN] = 0.0, 0.0
                                if known:
                                    opn = ear / s[BASE]
                        elif known and opn < P['close_ratio']:
                            s[CLOSED], s[RUN], s[MIN_OPEN], s[START] = 1.0, 1.0, opn, tick
                        elif known and opn >= P['open_ratio']:
                            rate = P['baseline_rise'] if ear > s[BASE] else P['baseline_rate']
                            s[BASE] = s[BASE] + np.float64(rate) * (ear - s[BASE])
                    if s[CLOSED] != 0.0:
                        r |= R_CLOSED
                        blink[b, f, e] = 1
                    elif s[HOLD] > 0.0:
                        r |= R_HOLD
                        s[HOLD] = s[HOLD] - 1.0
                reason[b, f, e] = r
                usable[b, f, e] = 1 if r == 0 else 0
                openness[b, f, e] = np.float32(opn)
        state[b, :, TICK] = state[b, :, TICK] + np.float64(n)
        count[b] = cnt
    return {'usable': usable, 'reason': reason, 'openness': openness, 'blink': blink}


# ---------------------------------------------------------------------------------------------------------------- test material
def eyelid_points(ear, width=30.0, centre=(100.0, 60.0), w=None):
    """Six eyelid points p1 .. p6 of an eye `width` pixels wide whose aspect ratio is `ear` (in exact arithmetic) -> float32 [6, 2 | 3]."""
    cx, cy = centre
    half = 0.5 * ear * width
    pts = [(cx - width / 2, cy), (cx - width / 6, cy - half), (cx + width / 6, cy - half), (cx + width / 2, cy), (cx + width / 6, cy + half),
           (cx - width / 6, cy + half)]
    a = np.array(pts, dtype=np.float32)
    if w is not None:
        a = np.concatenate([a, np.full((6, 1), w, dtype=np.float32)], axis=1)
    return a


def eyelid_trace(T, closures, open_ear=0.30, closed_ear=0.05, noise=0.01, seed=0, C=2):
    """contours [1, T, 2, 6, C] of both eyes (the right eye the left one's copy, 80 px to the right) with the aspect ratio open_ear
    +- noise, and closed_ear during each (first frame, frames) of `closures`."""
    rng = np.random.RandomState(seed)
    ear = open_ear + rng.uniform(-noise, noise, T)
    for t0, n in closures:
        ear[t0:t0 + n] = closed_ear + rng.uniform(0, noise, len(ear[t0:t0 + n]))
    out = np.zeros((1, T, 2, 6, C), dtype=np.float32)
    for t in range(T):
        for e in range(2):
            out[0, t, e] = eyelid_points(ear[t], centre=(100.0 + 80.0 * e, 60.0), w=None if C == 2 else 1.0)
    return out, ear


def translation_warp(dx, dy=0.0):
    return np.array([1.0, 0.0, dx, 0.0, 1.0, dy, 0.0, 0.0, 1.0], dtype=np.float32)



# the case the host and the GPU suites share: EyeGateSpec(blink=BlinkSpec(**CASE_BLINK), **CASE_SPEC), frames CASE_FRAME, patches CASE_PATCH
CASE_SPEC = dict(max_reproj_px=3.0, min_inliers=5, min_coverage=0.5, head_pitch=(-0.5, 0.5), head_yaw_left=(-0.6, 0.3), head_yaw_right=(-0.3, 0.6))
CASE_BLINK = dict(close_ratio=0.65, open_ratio=0.75, baseline_rate=0.02, baseline_rise=0.5, hold_frames=2, max_closed_frames=20)
CASE_FRAME, CASE_PATCH = (640, 480), (128, 64)
PREROLL = 10


def kernel_case(T, params, seed=3):
    """B = 3 streams x T frames with every kind of frame, after a pre-roll of 10 frames (8 open, 2 closed) through run() itself, so
    every stream arrives with both eyes closed, tick 10 and a baseline.  The store has 2 rows; stream 0's first is in use.
      stream 0  lengths T: both eyes reopen in frame 0 (the left blink is stored, the right one dropped), hold-off in frames 0, 1; frame 2
                usable, with a NaN contour (left) and a weight of 0 (right): unknown, which moves nothing; frame 3 a NaN rms; frame 4
                a zero warp and pose_valid 0 for the left eye; T = 70: the left eye closed in frames 60 .. 66, across the pass boundary
      stream 1  lengths 0 and a reset flag, NaN everywhere: the rows are cleared, nothing else happens
      stream 2  lengths max(1, T - 1): frame 0 still closed, with too few inliers, an rms above the bound, the left patch 3/4 outside the
                frame, the right eye's yaw out of range and its pose invalid; both eyes reopen in frame 1 (two rows), frame 3 usable;
                T = 70: the right eye closed from frame 10 to 40, longer than max_closed_frames: the baseline starts over in frame 30
    -> a dict: the arguments of run() (state, store, count, dropped are the pre-roll's, to be copied before use)."""
    B = 3
    rng = np.random.RandomState(seed)
    ear = 0.30 + rng.uniform(-0.01, 0.01, (B, PREROLL + T, 2))
    closed = np.zeros((B, PREROLL + T, 2), dtype=bool)
    closed[:, PREROLL - 2:PREROLL] = True
    closed[2, PREROLL] = True
    if T == 70:
        closed[0, PREROLL + 60:PREROLL + 67, 0] = True
        closed[2, PREROLL + 10:PREROLL + 41, 1] = True
    ear[closed] = 0.05 + rng.uniform(0, 0.01, int(closed.sum()))
    contours = np.zeros((B, PREROLL + T, 2, 6, 3), dtype=np.float32)
    for b in range(B):
        for t in range(PREROLL + T):
            for e in range(2):
                contours[b, t, e] = eyelid_points(ear[b, t, e], width=30.0 + b, centre=(100.0 + 80.0 * e + t % 3, 60.0 + b), w=1.0)
    state, store, count, dropped = fresh(B, 2)
    run(params, B, PREROLL, state, store, count, dropped, contours=contours[:, :PREROLL])
    assert (state[:, :, CLOSED] == 1).all() and (state[:, :, TICK] == PREROLL).all() and not count.any()
    store[0, 0] = (7.0, 8.0, 9.0, 0.5)
    count[0] = 1
    contours = contours[:, PREROLL:].copy()
    pose_valid = np.ones((B, T, 2), dtype=np.uint8)
    rms = rng.uniform(0.5, 2.0, (B, T)).astype(np.float32)
    inliers = rng.randint(5, 20, (B, T)).astype(np.uint8)
    base = np.array([1.1, 0.05, 100.0, -0.04, 0.95, 80.0, 1e-4, -2e-4, 1.0])
    warp = (base + rng.uniform(-1, 1, (2, B * T, 9)) * np.array([0.01, 0.01, 5, 0.01, 0.01, 5, 1e-5, 1e-5, 0])).astype(np.float32)
    h = rng.uniform(-0.25, 0.25, (2, B * T, 2)).astype(np.float32)
    q = lambda b, t: b * T + t
    if T > 2:
        contours[0, 2, 0, 4, 1] = np.nan
        contours[0, 2, 1, 1, 2] = 0.0
    if T > 3:
        rms[0, 3] = np.nan
    if T > 4:
        warp[0, q(0, 4)] = 0.0
        pose_valid[0, 4, 0] = 0
    for a in (contours, rms, warp[:, q(1, 0):q(1, T - 1) + 1], h[:, q(1, 0):q(1, T - 1) + 1]):
        (a[1] if a is contours or a is rms else a)[...] = np.nan
    inliers[2, 0], rms[2, 0] = 4, 3.5
    warp[0, q(2, 0), 2] = 600.0
    h[1, q(2, 0), 1] = 0.7
    pose_valid[2, 0, 1] = 0
    lengths = np.array([T, 0, max(1, T - 1)], dtype=np.int32)
    reset = np.array([0, 1, 0], dtype=np.int32)
    return dict(state=state, store=store, count=count, dropped=dropped, pose_valid=pose_valid, reproj_rms=rms, inliers=inliers, warp=warp, h=h,
                contours=contours, lengths=lengths, reset=reset, frame=CASE_FRAME, patch=CASE_PATCH)


def run_case(case, params, B=3):
    """run() on copies of the case's state and store -> (outputs, state, store, count, dropped)."""
    carried = [case[k].copy() for k in ('state', 'store', 'count', 'dropped')]
    T = case['pose_valid'].shape[1]
    out = run(params, B, T, *carried, **{k: v for k, v in case.items() if k not in ('state', 'store', 'count', 'dropped')})
    return (out,) + tuple(carried)


def case_is_rich(T, out, case, count, dropped):
    """What the shared case must show ON THE REFERENCE before a comparison with it means anything.  T = 1 has four delivered (frame,
    eye) cells -- two reopening, two still closed -- so it cannot also hold a usable eye; every other T must show everything."""
    live = np.arange(T)[None, :] < case['lengths'][:, None]
    reasons = out['reason'][live]
    bits = int(np.bitwise_or.reduce(reasons.reshape(-1)))
    stored, lost = int(count.sum() - case['count'].sum()), int(dropped.sum() - case['dropped'].sum())
    ok = bits == 127 and stored >= 1 and lost >= 1 and (out['usable'][live] == 0).any(axis=0).all()
    if T > 1:
        ok = ok and (out['usable'][live] == 1).any(axis=0).all()
    return bool(ok)
