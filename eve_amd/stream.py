"""EVEStream: EVE inference over videos longer than one clip, and over live cameras, with both networks' recurrent states
carried from one call to the next.

    stream = eve_amd.EVEStream(model, num_streams=B)      # model: an eve_amd.EVE in eval mode
    out = stream.step(chunk)                               # chunk: dict of [B, Tc, ...] GPU tensors, any Tc >= 1
    out = stream.step(chunk, lengths=[3, 1, 0, 3])         # ragged: stream b delivered only lengths[b] frames (see step)
    out = stream.step(chunk, eye_mask=usable)              # masked: usable [B, Tc, 2] marks the eyes to consume, frame by frame
    stream.reset([3])                                      # stream 3 starts from zero state at the next step()
    stream.step(dict(chunk, calibration_target=dots))      # collect per-person calibration samples (see "Calibration" below)
    fit = stream.fit_calibration(huber_mm=25.0)            # fit each eye's offset on the device; later steps apply it
    stream.step(dict(chunk, screen_calibration_target=dots))          # collect for the screen-space map ("Screen-space calibration")
    fit = stream.fit_screen_calibration(model='affine')    # fit it on the device; later steps correct their output point
    out = stream.step(chunk, events=eve_amd.GazeEventSpec(fps=60))   # + the filtered PoG, gaze velocity, fixation / saccade events
    rows = stream.fixations()                              # the completed fixations of every stream (see "Gaze events" below)
    out = stream.step(chunk, events=eve_amd.GazeEventSpec(fps=60), saccades=eve_amd.SaccadeSpec())   # + saccade_id, saccade_ms ("Saccades")
    rows = stream.saccades()                               # the accepted saccades: amplitude, duration, peak velocity, the fixations around them
    out = stream.step(chunk, events=eve_amd.GazeEventSpec(fps=60), pursuits=eve_amd.PursuitSpec())   # + gaze_class, pursuit_id, ... ("Smooth pursuit")
    rows = stream.pursuits()                               # the accepted pursuit episodes: amplitude, direction, velocities, path, gain
    out = stream.step(chunk, gate=eve_amd.EyeGateSpec(blink=eve_amd.BlinkSpec()))   # the mask made on the device (see "The eye gate" below)
    out = stream.step(chunk, history=eve_amd.GazeHistorySpec(fps=60))                # + the time-decayed map of where the gaze has been
    out = stream.step(dict(chunk, aoi_shapes=regions), aoi=eve_amd.AoiSpec(num_aois=8, fps=60))   # + which region is looked at ("Areas of interest")
    out = stream.step(chunk, pupil=eve_amd.PupilSpec(fps=60))          # + the validated, fused, baseline-corrected pupil size ("Pupillometry")
    out = stream.step(chunk, luminance=eve_amd.ScreenLuminanceSpec())  # + the screen's mean relative luminance, the pupil's light covariate ("Screen luminance")
    st = stream.get_state(); stream.set_state(st)          # reference layout, e.g. to resume a recording

For any split of a clip into chunks the concatenated outputs equal one eval pass of the whole clip from zero state
(EVE.forward with output_predictions): EyeNet's GRU / RNN / LSTM state and RefineNet's conv-RNN state are the only coupling
between frames, and they are handed from the last frame of one chunk to the first of the next.

The carried states live in fixed device buffers in the modules' own layout and dtype (EyeNet [2B, H] float32, the left eyes'
rows then the right ones'; RefineNet [B, 5, 8, C] NHWC), so a step converts nothing.  Each is zeroed where reset and committed
from the chunk's last frame by eve_stream_state_rows.  (EyeNet.stream_fused_tail runs the shipped EyeNet tail as one
eve_eye_tail_stream_fwd launch that updates its GRU state in place; it measured slower, so it is off by default.)

A ragged step (lengths=...) hands each stream's states over at its own frame count: eve_stream_state_rows_at commits from frame
lengths[b] - 1 (eve_eye_tail_stream_fwd_len for the fused tail) and leaves a stream with no frames alone.  The counts are a
device int32 [2B] filled from a pinned block like the reset flags, so the host never waits and one graph per chunk shape serves
every length pattern.  The chunk keeps its shape: frames past a stream's count cost what real ones cost (no compaction).

A masked step (eye_mask=..., skip_invalid_pose=True) skips frames in the middle of a chunk, per eye: one eve_stream_mask_plan
launch turns the mask (ANDed with the lengths and, on request, the pose form's pose_valid) into a stable partition per
sequence, eve_stream_permute_rows moves every sequence's usable frames to the front, the ragged machinery above runs with the
usable counts as lengths, and the per-frame results are moved back.  The binocular quantities of a frame with one usable eye
come from that eye alone (EVE._predict_sequence).  The mask is a graph input like the chunk: one masked graph per chunk shape.

With use_graph (the default) each distinct chunk shape is captured once into a hipGraph on one stream and replayed; the
chunk is copied into the graph's input buffers first.  Resets are device flags written by the host before the replay.  A
changed weight (load_state_dict, an optimiser step through torch) is detected through the parameters' versions, as the
modules' weight packs are, and the graphs are captured again.  Weights changed behind torch's back (a fused optimiser
kernel) need invalidate(), as the modules need invalidate_packs().

Calibration.  Every person's visual axis sits a few degrees off the optical axis EyeNet sees; the reference trains RefineNet
under random offsets of that kind (kappa_fake) for this reason.  An EVEStream can collect, fit and apply that offset per
stream and eye, all on the device and stream-ordered.  A chunk with calibration_target, float32 [B, Tc, 2] -- the dot the person
was asked to look at, in actual_screen_size pixels -- and optionally calibration_valid, bool or uint8 [B, Tc], makes the step
append what the fit needs of every usable (frame, eye) to this EVEStream's sample store (one eve_calib_append launch inside
the step and the graph; float64 [B, 2, C, 16], C = calibration_capacity; a full store drops and counts).  fit_calibration() fits
each eye's kappa = (pitch, yaw) by one eve_calib_fit launch, and from then on the step applies the stream's rows through the
offset path of eve_gaze_to_pog: <side>_g_initial, PoG_*_initial, g_initial, heatmap_initial and everything RefineNet derives
follow from the calibrated angles, the network's own angles appear as <side>_g_initial_raw, and the result gains calibrated,
bool [B].  A stream that is not calibrated keeps the bits of an uncalibrated EVEStream (a select per stream, not a kappa of
zero), and an EVEStream on which no calibration call was ever made issues exactly the launches it always issued.  Samples are
always collected from the raw angles, so collecting while calibrated does not compound.  The offset and the store belong to the
person, not to the clip: reset() touches neither, and get_state() / set_state() do not hold them (get_calibration /
set_calibration do).  Not offered: per-sample weights from the caller (entry 14 of a sample is reserved at 1.0), automatic or
continuous recalibration, gradients, application in EVE.forward.

Screen-space calibration.  What remains after kappa depends on the position on the screen -- a camera-to-screen transform a little
off, a head-pose dependent bias, a cornea that is not the average one -- and is what a tracker's five- or nine-dot procedure removes:
a low-order map of the OUTPUT point.  <out> is final with a RefineNet, else initial (the rule GazeEventSpec(source=None) uses).  With
(x, y) = PoG_px_<out>, u = 2x / W - 1, v = 2y / H - 1 over actual_screen_size and phi = (1, u, v, u*u, u*v, v*v), the models 'offset',
'affine' (default) and 'quadratic' use 1, 3 and 6 terms; the correction is coef[axis][term] in MILLIMETRES on the screen, and the
corrected pixel x + s_x * pixels_per_millimeter is clamped to the screen.  A chunk with screen_calibration_target, float32
[B, Tc, 2], and optionally screen_calibration_valid, bool or uint8 [B, Tc], makes the step append what the fit needs of every usable
frame (one eve_screen_calib_append launch after the point is known, inside the graph; float64 [B, C, 12], C =
screen_calibration_capacity, 96 bytes a row; a full store drops and counts) -- always from the UNCORRECTED point, so collecting while a
map is applied does not compound.  The keys are deliberately not calibration_target: kappa's collector reads the networks' raw
angles, this one the pipeline's output under whatever kappa is applied at that step, so the two rounds of dots are separate data (one
chunk may carry both), and A MAP BELONGS TO THE KAPPA IT WAS COLLECTED UNDER: fit kappa first, and after a new kappa collect and fit
the map again.  fit_screen_calibration() fits by one eve_screen_calib_fit launch (linear least squares by Cholesky, float64, fixed
summation order; with huber_mm re-weighted until no coefficient moves, at most 64 solves) and reports accuracy the way trackers do:
rms_mm, mean_mm, max_mm on the screen and mean_deg at the eye, for the corrected point and (with _raw) the uncorrected one.
evaluate_screen_calibration() reports the same for the STORED map over the current store and changes nothing: the validation pass
(clear_screen_calibration_samples, show other dots, collect, evaluate).  From the first fit or set_screen_calibration on, the step
runs one eve_screen_calib_apply launch right after the point it corrects: PoG_px_<out> is the corrected point, PoG_cm_<out> and g_<out>
are recomputed from it by the expressions _final_block uses, the uncorrected point appears as PoG_px_<out>_raw, and the result gains
screen_calibrated, bool [B]; heat maps, every *_initial key under a RefineNet, the per-eye angles and the kappa collector are
untouched.  The stage runs before the events stage and the render hook, so filtering, fixations and overlay markers that name
PoG_px_<out> see the corrected point.  A stream without a map (kind 0) keeps its bits, and an EVEStream on which none of these calls was
made and whose chunks carry no such key issues exactly the launches it always issued.  lengths, eye_mask, gate= and every camera and
screen form combine; collection honours lengths and the masked plan's valid.  Needs inv_camera_transformation, pixels_per_millimeter
and the origins (applying also millimeters_per_pixel and camera_transformation): ValueError otherwise, as for
screen_calibration_valid without its target.  reset(), get_state() and set_state() do not touch any of it (get_screen_calibration /
set_screen_calibration / clear_screen_calibration / clear_screen_calibration_samples / screen_calibration_counts /
screen_calibration_samples do).  tests/screen_calib_ref.py states the arithmetic, exact to the bit.  Not offered: per-sample weights
from the caller (entry 9 of a sample is reserved at 1.0), cubic or higher models, automatic recalibration, a gradient, EVE.forward.

Gaze events.  What comes out of the networks is a raw per-frame point of gaze, and every consumer of an eye tracker then smooths
it, differentiates it and cuts it into fixations and saccades -- on the host that is a sync per chunk and a loop per stream, with
state that has to survive chunk boundaries, ragged lengths, masked eyes and reset(): what an EVEStream owns.  step(chunk,
events=eve_amd.GazeEventSpec(...)) adds one eve_gaze_events launch at the end of the step and inside the graph: a one-euro filter
on the source PoG (PoG_px_filtered), the angular velocity of the gaze vector at the eye between consecutive samples
(gaze_velocity, degrees / second), a velocity-threshold label per frame (gaze_event: 1 fixation, 2 saccade, 0 none), the running
fixation (fixation_id, fixation_px, fixation_ms, fixating), and completed fixations appended to a per-stream store on the device
(float64 [B, fixation_capacity, 8]; fixations(), fixation_counts(), clear_fixations(), flush_fixations()).  The filter's and the
events' state is a float64 [B, 32] row per stream, carried from step to step like the recurrent states and reset through the same
device flags (get_event_state / set_event_state; get_state / set_state do not hold it).  Float64 throughout;
tests/gaze_events_ref.py states the arithmetic.  A step without events issues exactly the launches it always issued.  Not offered:
dispersion (I-DT) or other classifiers, windowed velocity, merging of adjacent fixations and retroactive relabelling,
a blink class, per-eye events, gradients, EVE.forward.  (Smooth pursuit, the third class: "Smooth pursuit" below.)

Saccades.  The events stage labels every frame, and only fixations leave it as events; saccades are the other half of every event
detector -- amplitude, duration, peak and mean velocity, the link fixation -> saccade -> fixation that is the scan path, an "in
saccade" flag for saccadic suppression, the main sequence -- and cannot be rebuilt from the step's results: the gaze vectors, the
sample flags and the sample times live inside the events launch, and an open saccade has to survive chunk boundaries, ragged lengths,
masked eyes and reset().  step(chunk, events=..., saccades=eve_amd.SaccadeSpec(...)) makes the events launch eve_gaze_events_ex, which
hands those three out (same kernel, same bits; they stay internal), and adds one eve_gaze_saccades launch right after it, before the
history stage, inside the graph.  A saccade opens at the sample before its first saccade frame and lands at its last; the next
fixation frame closes and judges it: more than max_missing frames inside it that were no sample -> interrupted, longer than
max_duration_s -> long, shorter than min_duration_s -> short, under min_amplitude_deg -> small, else accepted.  A gap, a restart of
the chain and reset() abort it.  The result gains saccade_id int32 [B, Tc] (-1 outside; ids run on over reset() and are handed out at
the onset, accepted or not) and saccade_ms float32 [B, Tc].  Per stream the launch keeps a float64 [B, 32] state row, a table float64
[B, 16] (accepted, sum amp, sum amp^2, sum peak, sum amp*peak, sum dur, sum amp*dur, max amp, max peak, aborted, small, short, long,
interrupted, 0, 0: the sums behind the main sequence, data.main_sequence()) and a store float64 [B, saccade_capacity, 16] (id, t_onset,
t_landing, n, x0, y0, x1, y1, amplitude_deg, peak_deg_s, mean_deg_s, prev_fixation_id, next_fixation_id, missing, 0, 0; a full store
drops and counts): saccades(), saccade_counts(), saccade_table(), clear_saccades(), get_saccade_state() / set_saccade_state();
get_state() / set_state() do not hold them.  reset() aborts the open saccade and starts the row afresh through the same device flags
(also before a step without saccades=); the id counter and the table stay.  There is no flush: an open saccade has no landing.  The
amplitude is the angle at the eye between the onset's and the landing's gaze vectors, so it is that of the point the velocity is
from: with velocity_from='filtered', the default, the one-euro filter's lag shortens it (8.9 / 9.2 / 9.5 degrees for a 10 degree
saccade at 30 / 60 / 120 fps on the scan path of tests/test_gaze_events_host.py; 9.9 .. 10.0 with 'raw').  The fixation ids a row
links to are the events stage's: a fixation that never reached min_fixation_s is in no store and still has its id.  An events step
without saccades= moves the chain on without the stage; the stream remembers, and one launch with no frames starts every row afresh
before the next saccades step.  Float64; tests/saccade_ref.py states the rules, and the device equals them bit for bit up to the
amplitude's atan2.  A step without saccades= issues exactly the launches it always issued, eve_gaze_events included, and allocates
nothing.  Not offered: direction angles (the endpoints are there), curvature or path length, glissades and post-saccadic
oscillation, microsaccades, per-eye saccades, retroactive merging, gradients, EVE.forward.

Smooth pursuit.  EVE's stimuli include videos, and on a moving target the eye neither fixates nor jumps: it follows at 2 .. 30 degrees
/ second, far below saccade_deg_s, so the events stage labels those frames fixations, fixation_px drifts behind the eye and
fixations() stores "fixations" hundreds of pixels long.  step(chunk, events=..., pursuits=eve_amd.PursuitSpec(...)) adds the third
class: the events launch is eve_gaze_events_ex (as for saccades=) and one eve_gaze_pursuits launch follows it -- after the saccade
launch where there is one, before the history stage, inside the graph.  Per stream the launch keeps the run of chained fixation
samples since the last saccade frame or restart (its last 32 in the state row; the samples of the first settle_s after a saccade
stay out, for the filter's creep after a landing) and looks at every new one over the window of the last window_s seconds: the
angle between the window's first and last gaze vector over its time (gaze_velocity_windowed), and that angle over the window's
path length, the sum of the events' velocities times their steps (gaze_straightness: 1 for straight motion, near 0 for jitter).
Where both reach their thresholds the frame is promoted: gaze_class 3 (else the events' label), pursuit_id, pursuit_ms.  The runs
of such frames are episodes: one opens at its first frame's window start (never before the end of the episode before it), ends at
its last frame, and is judged -- interrupted, short, small, or accepted -- when the next fixation frame that is no candidate, or a
saccade frame, arrives; a restart of the chain and reset() abort it, and one open at a chunk's end goes on in the next chunk.
Accepted episodes go to a table float64 [B, 16] (accepted, sum_dur, sum_amp, sum_path, sum_mean_v, max_peak, sum_gain, gain_n,
aborted, small, short, interrupted, 0 ...: data.pursuit_summary()) and a store float64 [B, pursuit_capacity, 20] (id, t_onset, t_end,
n, x0, y0, x1, y1, amplitude_deg, direction_deg, mean_deg_s, peak_deg_s, path_deg, fixation_id, missing, gain_n, mean_gain,
mean_error_px, 0, 0): pursuits(), pursuit_counts(), pursuit_table(), clear_pursuits(), get_pursuit_state() / set_pursuit_state().
With pursuit_target float32 [B, Tc, 2] in the chunk (the pursued object's screen position in pixels, NaN where none) every window
also has a gain -- the eye's displacement projected on the target's, over the target's (pursuit_gain; 1 is perfect tracking) -- and
the rows carry its mean and the mean distance to the target.  gaze_event, the fixation keys and the fixation store keep their bits:
a row's fixation_id names the "fixation" the episode lies in, for a consumer to discount.  The frames before a window fills are not
relabelled, so an episode's first min_window_s carry class 1 while its row's onset covers them.  Pursuit wants the filtered point:
with velocity_from='raw' jitter lowers the straightness and fragments episodes at high frame rates.  Float64; tests/pursuit_ref.py
states the rules, and the device equals them bit for bit up to the atan2 behind the angles.  A step without pursuits= issues exactly
the launches it always issued and allocates nothing.  Not offered: hysteresis, or merging episodes across catch-up saccades (the rows
carry what a host merge needs); retroactive relabelling; per-eye pursuit; vestibulo-ocular compensation; gradients; EVE.forward.

The eye gate.  The masked step keeps an unusable eye out of the states and the fused gaze, but it needs the mask, and what should
veto an eye -- pose_valid, face_reproj_rms, face_inliers, the derived warps and head angles, a closed lid -- are results of the same
step: a host that acts on them waits for the device every chunk, or is one chunk late.  step(chunk, gate=eve_amd.EyeGateSpec(...))
adds one eve_eye_gate launch between the pose derivation and eve_stream_mask_plan, inside the graph, whose verdict becomes the
step's eye_mask (ANDed into the caller's where there is one): a gated step is a masked step, and the scans, the fusion, the
calibration samples, the gaze events and the overlay follow through eye_valid / valid.  The result gains eye_gate_reason uint8
[B, Tc, 2] (bits: 1 pose, 2 reprojection, 4 inliers, 8 coverage, 16 head angle, 32 eyelid closed, 64 hold-off after a blink),
eye_openness float32 [B, Tc, 2] (the eyelid aspect ratio of the chunk's eye_contours over a baseline that follows the open eye; NaN
where unknown) and blink uint8 [B, Tc, 2]; completed blinks go to a per-stream store (float64 [B, blink_capacity, 4]: eye, first
tick, last tick, minimum openness; blinks(), blink_counts(), clear_blinks()).  The blink state is a float64 [B, 2, 8] row per eye,
carried from step to step and reset through the same device flags, also before a step without gate (get_gate_state /
set_gate_state; get_state / set_state do not hold it).  Float64 throughout; tests/eye_gate_ref.py states the arithmetic.  A step
without gate issues exactly the launches it always issued.  Not offered: adaptive thresholds learnt per person, a closure announced
before its first closed frame, blink times in seconds, a mid-chunk reset of stale recurrent state after a long gap, coverage
through the lens model, gradients, EVE.forward.

Gaze history.  "Where has this person been looking" -- over the last seconds, or over the whole session -- is the picture every
consumer of an eye tracker builds next (an attention map, a dwell map, a fixation heat map), and what the reference's
EVE.forward(create_images=True) returns as initial_gaze_history / refined_gaze_history: per clip the sum over frames of validity *
decay_per_ms^(ms before the last frame) * heat map.  That sum is the recurrence M_t = decay^(dt_ms) * M_{t-1} + w_t * G_t, and a map
per stream that survives chunk boundaries, ragged lengths, masked eyes and reset() is state of the kind an EVEStream owns.
step(chunk, history=eve_amd.GazeHistorySpec(...)) -- one spec, or two with distinct names -- adds two launches per spec after the
events stage and before the render hook, inside the graph: eve_gaze_history_plan (a wavefront per stream walks the time chain and
writes one coefficient row per frame) and eve_gaze_history_update (each map tile is loaded once, taken through the chunk's frames in
registers and stored once).  The result gains <name>, float32 [B, MH, MW] (a copy of the carried map after the stream's last consumed
frame), and with per_frame <name>_frames [B, Tc, MH, MW].  The source is a point of gaze of the step (PoG_px_initial / _final; with
events= PoG_px_filtered or fixation_px, the latter with valid_key='fixating' the fixation heat map) rendered as a Gaussian of sigma map
pixels, or heatmap_final, the network's own maps (the reference's refined_gaze_history); weight='seconds' with decay_per_ms=1 gives
a dwell map in seconds.  Time is the chunk's frame_time or frames / spec.fps, as for the events.  A frame that is not usable (lengths,
the masked plan's valid, valid_key, a non-finite point) decays the map and deposits nothing; one whose time is not finite or runs
backwards is ignored.  The map and its float64 [B, 8] time-chain row are carried from step to step, cleared by reset() through the same
device flags (also before a step that does not run the spec), and tied to the spec: the same name under another spec is refused until
clear_gaze_history().  gaze_history(), clear_gaze_history(), get_gaze_history_state() / set_gaze_history_state(); get_state() /
set_state() do not hold them.  OverlaySpec(heat_key=<name>) blends a per_frame map in place of heatmap_final.  Float64 arithmetic on a
float32 map that is rounded after every frame, with an exp the contract owns: tests/gaze_history_ref.py states it, and the device
equals it bit for bit, so a clip cut into chunks gives the bits of one pass.  A step without history= issues exactly the launches it
always issued and allocates nothing.  Not offered: per-eye maps, a windowed history (as opposed to the decayed one), anisotropic or
screen-millimetre sigmas, gradients, EVE.forward (its create_images path keeps the torch restatement), maps larger than 2048 per axis.

Areas of interest.  WHAT is the person looking at, for how long, how often, in which order -- the first question a consumer asks of a
tracker -- is a hit test per frame and a small state machine per stream, whose state has to survive chunk boundaries, ragged lengths,
masked eyes and reset(): what an EVEStream owns.  step(chunk, aoi=eve_amd.AoiSpec(num_aois=A, ...)) adds one eve_gaze_aoi launch after
the events and history stages and before the render hook, inside the graph.  The regions come with the chunk as aoi_shapes, float32
[B, A, 36] or -- for stimuli that move, a video or a scrolling page -- [B, Tc, A, 36], a graph input like the rest of the chunk, so one
graph serves every layout of the regions; data.aoi_shapes builds a table from rectangles (half open), ellipses and polygons of up to
16 vertices (even-odd), the order of the rows being the z-order.  The point is a point of gaze of the step (PoG_px_initial / _final,
the screen-calibrated one where a map is applied; with events= PoG_px_filtered or fixation_px, the latter with valid_key='fixating'
the fixation-based analysis).  The result gains <name>_id int32 [B, Tc] (the lowest row that contains the point, -1 none, -2 the frame
is not a sample), <name>_mask int64 [B, Tc] (bit a: row a contains it) and <name>_visit_ms float32 [B, Tc].  Per stream the launch
keeps a dwell table float64 [B, A + 1, 8] (dwell_s, samples, visits, t_first_entry, t_last, fixations, t_first_fixation, 0; row A: no AOI),
a transition matrix int32 [B, A + 1, A] (row A: the first visit since a reset; the diagonal: revisits) and a store of completed visits
float64 [B, visit_capacity, 8] (aoi, t_enter, t_last, samples, fixations, visit_index, 0, 0; a full store drops and counts):
aoi_table(), aoi_transitions(), aoi_visits(), aoi_visit_counts(), clear_aoi(), flush_aoi_visits().  A frame is a sample iff it was
delivered (lengths), is valid (eye_mask, gate=, skip_invalid_pose), its valid_key holds, its point and its time are finite and the
time is later than the last sample's; two samples more than max_gap_s apart are not connected.  With events= in the same step (or
use_fixations=True) fixations are counted per AOI and per visit from fixation_id / fixating.  Time is the chunk's frame_time or
frames / spec.fps, as for the events.  The float64 [B, 16] state row is carried from step to step and reset through the same device
flags (also before a step without aoi=): reset() closes the open visit into the store and starts the row afresh, only the visit
counter runs on; the tallies stay -- they are a readout like the fixation store, cleared by clear_aoi() -- and are tied to their spec
as a history map is.  get_aoi_state() / set_aoi_state(); get_state() / set_state() do not hold them.  Float64, + - * / and comparisons
only: tests/aoi_ref.py states it, and the device equals it bit for bit, so a clip cut into chunks gives the bits of one pass.  A step
without aoi= issues exactly the launches it always issued and allocates nothing.  Not offered: label-map AOIs, minimum visit
durations or border hysteresis, per-eye AOIs, polygon margins, AOI outlines in the overlay, gradients, EVE.forward.

Pupillometry.  EyeNet's second head, the pupil size per eye, leaves the step as the network wrote it: unspecified at unusable eyes,
noisy, unfused, without a baseline.  step(chunk, pupil=eve_amd.PupilSpec(...)) adds one eve_pupil_track launch after the AOI stage and
before the render hook, inside the graph, over the step's own <side>_pupil_size and -- on a masked or gated step -- the mask plan's
eye_valid, so what the mask, the gate, a blink or its hold-off withheld is withheld here too.  Per frame and eye a size is accepted
iff it was delivered, is finite, lies in min_mm .. max_mm and does not move faster than max_speed_mm_s against that eye's last
accepted size (the dilation-speed criterion of Kret & Sjak-Shie 2019 with a fixed bound; after max_gap_s the eye is re-admitted
untested).  The accepted eyes are fused through a running left - right offset, so the trace does not step when one eye drops out;
the fused size is low-passed (cutoff_hz), optionally corrected for light -- the chunk's pupil_luminance, float32 [B, Tc], is low-passed
with light_tau_s and, once a gain is set (set_pupil_light_response / fit_pupil_light_response), gain * (Lf - ref) is taken off --
and referred to a baseline: the running mean of the samples the chunk marks in pupil_baseline, bool / uint8 [B, Tc] (a new run of
marks starts a new baseline), or without marks a slow follower (baseline_tau_s).  The result gains <name>_mm, _raw_mm, _velocity,
_change_mm, _change_pct float32 [B, Tc] (NaN where the frame is no sample), _valid and _event uint8 [B, Tc] (1 dilating, 2
constricting) and _eye_used, _eye_reason uint8 [B, Tc, 2] (1 withheld, 2 not finite, 4 range, 8 speed).  Per stream the launch keeps a
table float64 [B, 24] (pupil_table() names the entries), and a store of dilation / constriction episodes float64 [B,
episode_capacity, 8] (phase, t_start, t_end, d_start, d_end, peak |velocity|, samples, Lf at the start; a full store drops and
counts): pupil_episodes(), pupil_episode_counts(), clear_pupil(), flush_pupil_episodes().  Both chunk keys are graph inputs, their
presence part of the graph's key.  reset() closes the open episode and starts the float64 [B, 32] state row afresh (only the episode
counter runs on), also before a step without pupil=; the table and the light response stay, tied to their spec.  get_pupil_state() /
set_pupil_state(); get_state() / set_state() do not hold them.  Float64, + - * /, abs and comparisons only: tests/pupil_ref.py states
it, and the device equals it bit for bit, so a clip cut into chunks gives the bits of one pass.  A step without pupil= issues exactly
the launches it always issued and allocates nothing.  Not offered: non-causal blink padding and interpolation across gaps,
foreshortening correction, per-eye filtered traces, wavelet indices (IPA / LHIPA), per-fixation or per-AOI pupil means, the overlay,
gradients, EVE.forward.

Screen luminance.  On a screen-based tracker the pupil's response to the screen's light is the largest confound of the pupil trace,
and the capture it follows is already in the step's input.  step(chunk, luminance=eve_amd.ScreenLuminanceSpec(...)) adds one
eve_screen_luminance launch after the AOI stage and before the pupil stage, inside the graph, over the capture where it lies (any
screen key; screen_surface through refine_net.screen_layout): every visible pixel is converted, linearised through the display's
response table (sRGB, a power law or a measured curve), weighted (Rec.709) and summed in integers -- over the whole screen, <name>
float32 [B, Tc], and over up to four discs of radii_px actual_screen_size pixels around the spec's source point, <name>_gaze [B, Tc,
R].  to_pupil weighs the columns into <name>_covariate, which pupil= in the same step takes as its luminance (ValueError with
pupil_luminance in the chunk too).  The whole screen follows lengths only; the discs also the masked step's valid and valid_key.  What
is not delivered, a disc without a valid centre and a disc off the screen are NaN, a light sample the pupil stage ignores.  The mean
of the linearised pixels is not the linearised mean: a one-pixel checkerboard has 0.5, its mean byte 0.216, so the stage reads the
capture and not RefineNet's resized screen.  The response table goes to the device before any capture, cached per spec; the spec by
value is part of the graph's key; the stage carries no state.  Integers up to one float64 division: tests/screen_luminance_ref.py
states it, and the device equals it bit for bit.  A step without luminance= issues exactly the launches it always issued.  Not
offered: continuous (eccentricity-weighted) kernels beyond concentric discs, per-AOI luminance, 10-bit arithmetic, ambient light, the
camera image's luminance, the overlay, gradients, EVE.forward.
"""
from collections import namedtuple

import numpy as np
import torch

from .eye_net import eye_input, face_landmarks_key, has_pose_form
from .kernels import default_kernels

_WARMUP_STREAMS = {}

# the lazily made buffer groups (EVEStream._group): a sample store of either calibration, and what the events and the gate carry
SampleStore = namedtuple('SampleStore', 'samples count dropped')
StageBuffers = namedtuple('StageBuffers', 'state store count dropped')
AoiBuffers = namedtuple('AoiBuffers', 'state table trans visits count dropped')      # what eve_gaze_aoi carries, per AoiSpec name
PupilBuffers = namedtuple('PupilBuffers', 'state table light store count dropped')    # what eve_pupil_track carries, per PupilSpec name
SaccadeBuffers = namedtuple('SaccadeBuffers', 'state table store count dropped')      # what eve_gaze_saccades carries
PursuitBuffers = namedtuple('PursuitBuffers', 'state table store count dropped')      # what eve_gaze_pursuits carries


def _module_key(m):
    return (m.compute_dtype,) + tuple((p.data_ptr(), p._version) for p in m.parameters())


def _capacity(name, value):
    if isinstance(value, bool) or not isinstance(value, int) or value < 1:
        raise ValueError('%s must be an integer >= 1, got %r' % (name, value))
    return value


class EVEStream(object):
    def __init__(self, model, num_streams, use_graph=True, calibration_capacity=1024, fixation_capacity=256, blink_capacity=256,
                 screen_calibration_capacity=1024, visit_capacity=256, episode_capacity=256, saccade_capacity=256,
                 pursuit_capacity=256):
        if model.training:
            raise ValueError('EVEStream runs inference only: call model.eval() first')
        self.model = model
        self.num_streams = B = int(num_streams)
        if B < 1:
            raise ValueError('num_streams must be >= 1')
        self.device = next(model.parameters()).device
        if use_graph and self.device.type != 'cuda':
            raise ValueError('use_graph=True needs the model on the GPU')
        self.use_graph = bool(use_graph)
        self._eye = model.eye_net._stream_state_buffers(B, self.device)
        self._ref = model.refine_net._stream_state_buffers(B, self.device) if model.refine_net is not None else []
        self._flags = torch.zeros((2 * B,), dtype=torch.int32, device=self.device)   # stream b's reset flag at b and B + b
        self._flags_set = False
        self._lengths = torch.zeros((2 * B,), dtype=torch.int32, device=self.device)  # a ragged step's frame counts, laid out like _flags
        self._pose_gate = torch.ones((1,), dtype=torch.bool, device=self.device)     # False: a masked step ANDs pose_valid into its mask
        self._pose_gate_host = True
        self._pending = None                     # host bool [B]: resets requested for the next step
        # the face-landmark form's carried head pose, float64 (R row-major, t, has_pose) per stream: eve_face_pose_solve reads and
        # writes it inside the step (and the graph), and clears it where the reset flag is set
        self._face_pose = torch.zeros((B, 13), dtype=torch.float64, device=self.device)
        # per-person calibration: the sample store (eve_calib_append appends inside the step), each eye's kappa row and flag
        # (eve_calib_fit writes them; a stream is calibrated where both flags are set).  _calib_apply: a fit or a set_calibration
        # has happened, so the steps run the applying graphs.
        self.calibration_capacity = _capacity('calibration_capacity', calibration_capacity)
        self._calib_store = None                 # made at the first collecting step or calibration call: B * 2 * C * 128 bytes
        self._calib_kappa = torch.zeros((B, 2, 2), dtype=torch.float32, device=self.device)
        self._calib_ok = torch.zeros((B, 2), dtype=torch.uint8, device=self.device)
        self._calib_apply = False
        # the screen-space map: the sample store (eve_screen_calib_append appends inside the step), each stream's coefficients
        # (axis, term) in millimetres and its kind byte (0 none, 1 offset, 2 affine, 3 quadratic; eve_screen_calib_fit writes them).
        # _screen_apply: a fit or a set_screen_calibration has happened, so the steps run the applying graphs.
        self.screen_calibration_capacity = _capacity('screen_calibration_capacity', screen_calibration_capacity)
        self._screen_store = None                # made at the first collecting step or screen calibration call: B * C * 96 bytes
        self._screen_coef = torch.zeros((B, 2, 6), dtype=torch.float64, device=self.device)
        self._screen_kind = torch.zeros((B,), dtype=torch.uint8, device=self.device)
        self._screen_apply = False
        # gaze events (step(chunk, events=spec)): the filter's and the running fixation's state row per stream, the store of completed
        # fixations and its counters -- eve_gaze_events reads and writes them inside the step (and the graph)
        self.fixation_capacity = _capacity('fixation_capacity', fixation_capacity)
        self._events = None                      # made at the first events step or fixation call: (state, store, count, dropped)
        self._events_spec = None                 # the spec of the last events step: what closes a fixation outside a step
        # saccades (step(chunk, events=..., saccades=spec)): the open saccade's state row, the table of tallies, the store of accepted
        # saccades and its counters -- eve_gaze_saccades reads and writes them inside the step (and the graph).  _saccades_stale: the
        # events chain has moved without the stage since, so the row is brought back in step before the next saccades step
        self.saccade_capacity = _capacity('saccade_capacity', saccade_capacity)
        self._saccades = None                    # made at the first saccades step or saccade call: (state, table, store, count, dropped)
        self._saccades_spec = None               # the spec of the last saccades step: the scalars of a launch with no frames
        self._saccades_stale = False
        # smooth pursuit (step(chunk, events=..., pursuits=spec)): the run's ring and the open episode's state row, the table of tallies,
        # the store of accepted episodes and its counters -- eve_gaze_pursuits reads and writes them inside the step (and the graph).
        # _pursuits_stale: as _saccades_stale
        self.pursuit_capacity = _capacity('pursuit_capacity', pursuit_capacity)
        self._pursuits = None                    # made at the first pursuits step or pursuit call: (state, table, store, count, dropped)
        self._pursuits_spec = None               # the spec of the last pursuits step: the scalars of a launch with no frames
        self._pursuits_stale = False
        # the eye gate (step(chunk, gate=spec)): each eye's blink state row, the store of completed blinks and its counters --
        # eve_eye_gate reads and writes them inside the step (and the graph)
        self.blink_capacity = _capacity('blink_capacity', blink_capacity)
        self._gate = None                        # made at the first gated step or blink call: (state, store, count, dropped)
        # the gaze history (step(chunk, history=spec)): name -> {'spec', 'P' (the launches' scalars), 'state' float64 [B, 8], 'maps'
        # float32 [B, MH, MW], 'free'} -- the two eve_gaze_history launches read and write them inside the step (and the graph)
        self._history = {}
        # areas of interest (step(chunk, aoi=spec)): name -> {'spec', 'buffers' (an AoiBuffers: the state row, the dwell table, the
        # transitions, the visit store and its counters), 'free'} -- eve_gaze_aoi reads and writes them inside the step (and the graph)
        self.visit_capacity = _capacity('visit_capacity', visit_capacity)
        self._aoi = {}
        # pupillometry (step(chunk, pupil=spec)): name -> {'spec', 'buffers' (a PupilBuffers: the state row, the table, the light
        # response, the episode store and its counters), 'free'} -- eve_pupil_track reads and writes them inside the step (and the graph)
        self.episode_capacity = _capacity('episode_capacity', episode_capacity)
        self._pupil = {}
        # screen luminance (step(chunk, luminance=spec)): the response tables on the device, by spec key -- made before any capture, as
        # the overlay's marker tables are; the stage carries no state
        self._luminance_tables = {}
        self._graphs = {}
        self._graphs_key = None
        self._render_tables = {}                 # OverlaySpec.key() -> its marker table, int32 [M, 4] on the device

    # ------------------------------------------------------------------ state
    _GROUPS = ('_calib_store', '_events', '_gate', '_screen_store', '_saccades', '_pursuits')      # the attributes _group() may fill: None until first use

    def _group(self, attr, kind, *buffers):
        """The lazily made buffer group self.<attr>, a `kind` namedtuple of zeroed device tensors, one per (shape, dtype) -- made at
        the first call, which the step's checks place before any capture.  Every group is named in _GROUPS, so _carried() holds it."""
        assert attr in self._GROUPS
        if getattr(self, attr) is None:
            setattr(self, attr, kind(*(torch.zeros(shape, dtype=dtype, device=self.device) for shape, dtype in buffers)))
        return getattr(self, attr)

    def _carried(self):
        """Every tensor a step may write, as they exist now: what _capture's two warm-up steps must put back.  The recurrent states;
        the face-landmark form's head pose; kappa and its flags; both calibrations' sample stores and counters (the warm-up steps of
        a collecting graph would otherwise append every sample three times); the gaze events' state, store and counters (a capture
        would otherwise tick the filter three times); the saccades' state row, table, store and counters; the pursuits' likewise; the eye gate's ticks, baselines and blinks; every gaze history's time chain
        and map; every AOI spec's state row, tallies and visit store; every pupil spec's state row, table, light response and
        episode store.  A carried buffer that is not returned here corrupts its state under use_graph only, and only on the first
        step of a chunk shape: new ones are made by _group(), by _history_entry(), by _aoi_entry() or by _pupil_entry(), and are
        then here."""
        states = [t for s_ in self._eye + self._ref for t in (s_ if isinstance(s_, tuple) else (s_,))]
        groups = [t for attr in self._GROUPS for t in (getattr(self, attr) or ())]
        return states + [self._face_pose, self._calib_kappa, self._calib_ok] + groups + \
            [t for e in self._history.values() for t in (e['state'], e['maps'])] + [t for e in self._aoi.values() for t in e['buffers']] + \
            [t for e in self._pupil.values() for t in e['buffers']]

    @staticmethod
    def _zero_where(mask, *tensors):
        """Zero the streams' rows of each tensor where mask, a bool [B] device tensor, holds: on the device, the host does not wait."""
        for t in tensors:
            t.copy_(torch.where(mask.reshape((-1,) + (1,) * (t.dim() - 1)), torch.zeros_like(t), t))

    def _pinned(self, host):
        """A host tensor about to be copied to the device: with the model on the GPU a pinned block of torch's host allocator, so the
        copy is asynchronous and the block is not reused before it has run.  (Resets, lengths and masks go this way and are never
        baked into a graph.)"""
        return host.pin_memory() if self.device.type == 'cuda' else host

    def reset(self, streams=None):
        """Start the given streams (None = all; else indices, or a bool mask of length num_streams) from zero state at the
        next step().  Resets requested before one step accumulate.  A stream that has run the eye gate (step(gate=...)) has both
        eyes' blink rows and its tick cleared; an eye closed at that moment stores no blink.  A stream that has run gaze events (step(events=...)) closes its
        open fixation into the store -- if it lasted min_fixation_s -- and starts its filter, its events and its frame count afresh,
        by the same device flags; only its fixation id counter runs on, so ids stay unique within a recording.  A stream that has run the saccade stage (step(saccades=...)) aborts its open saccade -- tallied, nothing
        stored -- and starts that row afresh; its saccade id counter and its table run on.  A stream that has run the pursuit stage (step(pursuits=...)) likewise aborts its open episode and empties its run; its
        pursuit id counter and its table run on.  The per-person calibration -- each eye's kappa and the
        sample store -- is not touched: it belongs to the person, not to the clip (clear_calibration,
        clear_calibration_samples); neither are the screen-space map and its sample store (clear_screen_calibration,
        clear_screen_calibration_samples)."""
        m = np.zeros(self.num_streams, dtype=bool) if self._pending is None else self._pending
        m |= self._stream_mask(streams, 'reset')
        self._pending = m

    def _stream_mask(self, streams, where):
        """None (all), indices, or a bool mask of length num_streams -> numpy bool [B]."""
        B = self.num_streams
        m = np.zeros(B, dtype=bool)
        if streams is None:
            m[:] = True
        else:
            a = streams.detach().cpu().numpy() if torch.is_tensor(streams) else np.asarray(streams)
            if a.dtype == bool:
                if a.shape != (B,):
                    raise ValueError('%s: a mask needs num_streams (%d) entries' % (where, B))
                m |= a
            else:
                idx = a.astype(np.int64).reshape(-1)
                if idx.size and (idx.min() < -B or idx.max() >= B):
                    raise IndexError('%s: stream index out of range' % where)
                m[idx] = True
        return m

    # ------------------------------------------------------------------ calibration
    def _store(self):
        B, C = self.num_streams, self.calibration_capacity
        return self._group('_calib_store', SampleStore, ((B, 2, C, 16), torch.float64), ((B, 2), torch.int32), ((B, 2), torch.int32))

    def _device_mask(self, streams, where):
        return self._pinned(torch.from_numpy(self._stream_mask(streams, where))).to(self.device, non_blocking=True)

    def fit_calibration(self, streams=None, huber_mm=None, min_samples=5):
        """Fit the offset kappa = (pitch, yaw) of both eyes of the given streams (None = all; indices or a bool mask) to the samples
        collected so far: one eve_calib_fit launch, a wavefront per (stream, eye), Levenberg-Marquardt from kappa = 0 on every call
        (a refit never depends on history) on sum rho(|PoG_i(kappa) - target_i|) in millimetres on the screen -- rho the square,
        or with huber_mm a Huber loss of that many millimetres, which keeps a few frames in which the person looked elsewhere
        from tilting the result.  -> a dict of device tensors (the host does not wait): kappa float64 [B, 2, 2] (stream, eye,
        (pitch, yaw)), rms_mm float64 [B, 2] over all used samples, used and inliers int32 [B, 2] (the samples within huber_mm;
        used without the loss), ok bool [B, 2], calibrated bool [B].  ok is False -- and that eye's stored kappa and flag stay what
        they were -- with fewer than min_samples samples, a system that is not positive definite, no convergence, or |kappa|
        above 0.35 rad (20 degrees, four times any physiological offset: a divergence guard).  A stream is calibrated when both
        of its eyes have been fitted (or set); streams not named are left alone and report ok False.  The following steps apply
        the stored rows (a new graph per chunk shape).  tests/calib_ref.py states the fit in numpy."""
        from .data import check_huber_mm, check_min_samples
        huber_mm, min_samples = check_huber_mm(huber_mm, 'fit_calibration'), check_min_samples(min_samples, 'fit_calibration')
        B, C = self.num_streams, self.calibration_capacity
        select = None if streams is None else self._device_mask(streams, 'fit_calibration')[:, None].expand(B, 2).to(torch.uint8).reshape(-1).contiguous()
        samples, count, _ = self._store()
        kappa, rms, used, inliers, ok = default_kernels().calib_fit(
            samples.view(2 * B, C, 16), count.view(-1), select, huber_mm, min_samples, self._calib_kappa.view(2 * B, 2), self._calib_ok.view(-1))
        self._calib_apply = True
        return {'kappa': kappa.view(B, 2, 2), 'rms_mm': rms.view(B, 2), 'used': used.view(B, 2), 'inliers': inliers.view(B, 2),
                'ok': ok.view(B, 2) != 0, 'calibrated': (self._calib_ok != 0).all(dim=1)}

    def get_calibration(self):
        """The stored offsets (fresh tensors): kappa float32 [B, 2, 2] (stream, eye, (pitch, yaw)) -- the rows the steps apply --
        and calibrated bool [B].  Rows of eyes never fitted or set are zero."""
        return self._calib_kappa.clone(), (self._calib_ok != 0).all(dim=1)

    def set_calibration(self, kappa, streams=None):
        """Load offsets known from an earlier session: kappa [B, 2, 2] in get_calibration()'s layout (converted to float32; the
        rows of the given streams are used, None = all), which become calibrated.  Values are not judged."""
        B = self.num_streams
        kappa = torch.as_tensor(kappa, dtype=torch.float32).to(self.device)
        if tuple(kappa.shape) != (B, 2, 2):
            raise ValueError('set_calibration: kappa must be [%d, 2, 2] (stream, eye, (pitch, yaw)), got %s' % (B, tuple(kappa.shape)))
        m = self._device_mask(streams, 'set_calibration')
        self._calib_kappa.copy_(torch.where(m[:, None, None], kappa, self._calib_kappa))
        self._calib_ok.copy_(torch.where(m[:, None], torch.ones_like(self._calib_ok), self._calib_ok))
        self._calib_apply = True

    def clear_calibration(self, streams=None):
        """Forget the offsets of the given streams (None = all): they are uncalibrated again and get the plain bits.  The sample
        store stays."""
        self._zero_where(self._device_mask(streams, 'clear_calibration'), self._calib_kappa, self._calib_ok)
        if streams is None:
            self._calib_apply = False            # nothing left to apply: back to the launches of an uncalibrated EVEStream

    def clear_calibration_samples(self, streams=None):
        """Empty the sample store of the given streams (None = all), both eyes, and their dropped counters."""
        if self._calib_store is None:
            self._stream_mask(streams, 'clear_calibration_samples')
            return
        self._zero_where(self._device_mask(streams, 'clear_calibration_samples'), self._calib_store.count, self._calib_store.dropped)

    def calibration_counts(self):
        """-> (count, dropped), int32 [B, 2] device tensors (fresh): the samples each (stream, eye) holds, and those a full store
        (calibration_capacity) turned away."""
        _, count, dropped = self._store()
        return count.clone(), dropped.clone()

    def calibration_samples(self):
        """The sample store itself, float64 [B, 2, C, 16] (fresh): rows 0 .. count - 1 of (stream, eye) in the order the frames
        came, in the layout of data.calibration_samples / data.fit_gaze_offset."""
        return self._store()[0].clone()

    # ------------------------------------------------------------------ screen-space calibration
    def _screen_samples(self):
        B, C = self.num_streams, self.screen_calibration_capacity
        return self._group('_screen_store', SampleStore, ((B, C, 12), torch.float64), ((B,), torch.int32), ((B,), torch.int32))

    def _screen_result(self, res):
        from .data import SCREEN_CALIB_REPORT
        coef, report, used, inliers, solves, ok = res
        out = {'coef': coef, 'kind': self._screen_kind.clone(), 'ok': ok != 0, 'used': used, 'inliers': inliers, 'solves': solves,
               'screen_calibrated': self._screen_kind != 0}
        out.update({name: report[:, i] for i, name in enumerate(SCREEN_CALIB_REPORT)})
        return out

    def fit_screen_calibration(self, streams=None, model='affine', huber_mm=None, min_samples=None, max_shift_mm=100.0):
        """Fit the screen-space map of the given streams (None = all; indices or a bool mask) to the samples collected so far: one
        eve_screen_calib_fit launch, a wavefront per stream.  model: 'offset' (one constant shift), 'affine' (1, u, v: the default) or
        'quadratic' (+ u*u, u*v, v*v), u, v the output point over the screen in -1 .. 1; the map gives the correction in millimetres
        that brings the pipeline's output point onto the dots -- linear least squares, or with huber_mm a Huber loss of that many
        millimetres by re-weighting (at most 64 solves), which keeps frames in which the person looked elsewhere from bending the
        map.  -> a dict of device tensors (the host does not wait): coef float64 [B, 2, 6] (axis, term; millimetres), kind uint8
        [B] (the stored kinds after the fit), ok bool [B], used, inliers, solves int32 [B], the accuracy report float64 [B] --
        rms_mm, mean_mm, max_mm, mean_deg (the angle at the eye) of the corrected point against the dots, and rms_mm_raw,
        mean_mm_raw, max_mm_raw, mean_deg_raw of the uncorrected one -- and screen_calibrated bool [B].  ok is False -- and the
        stream's stored map stays what it was -- with fewer usable samples than max(min_samples, the model's terms), dots that do
        not determine the model (on one line for 'affine'; fewer than six positions, or a 5 x 1 row, for 'quadratic'), no
        convergence, or a correction above max_shift_mm at a sample (a divergence guard).  Streams not named are left alone and
        report ok False.  The following steps apply the stored maps (a new graph per chunk shape).  A map belongs to the kappa it
        was collected under: after fit_calibration / set_calibration / clear_calibration collect and fit it again.
        tests/screen_calib_ref.py states the fit in numpy."""
        from .data import check_huber_mm, check_max_shift_mm, check_screen_min_samples, check_screen_model
        kind = check_screen_model(model, 'fit_screen_calibration')
        huber_mm, max_shift_mm = check_huber_mm(huber_mm, 'fit_screen_calibration'), check_max_shift_mm(max_shift_mm, 'fit_screen_calibration')
        min_samples = check_screen_min_samples(min_samples, 'fit_screen_calibration')
        select = None if streams is None else self._device_mask(streams, 'fit_screen_calibration').to(torch.uint8).contiguous()
        samples, count, _ = self._screen_samples()
        res = default_kernels().screen_calib_fit(samples, count, select, 0, kind, huber_mm, min_samples, max_shift_mm,
                                                 self._screen_coef, self._screen_kind)
        self._screen_apply = True
        return self._screen_result(res)

    def evaluate_screen_calibration(self, streams=None):
        """The validation pass: the accuracy of the STORED maps over the samples the store holds now -- clear the samples
        (clear_screen_calibration_samples), show other dots, collect, call this.  One eve_screen_calib_fit launch in mode 1; nothing
        is solved and nothing changes.  -> fit_screen_calibration's dict (solves 0, inliers = used, ok where the stream holds a
        sample); a stream without a map reports the raw numbers in both sets."""
        select = None if streams is None else self._device_mask(streams, 'evaluate_screen_calibration').to(torch.uint8).contiguous()
        samples, count, _ = self._screen_samples()
        return self._screen_result(default_kernels().screen_calib_fit(samples, count, select, 1, 0, None, 1, 100.0,
                                                                      self._screen_coef, self._screen_kind))

    def get_screen_calibration(self):
        """The stored maps (fresh tensors): coef float64 [B, 2, 6] (axis, term; millimetres) and kind uint8 [B] (0 none, 1 offset, 2
        affine, 3 quadratic)."""
        return self._screen_coef.clone(), self._screen_kind.clone()

    def set_screen_calibration(self, coef, kind, streams=None):
        """Load maps known from an earlier session, in get_screen_calibration()'s layout: coef [B, 2, 6] (converted to float64), kind
        B integers in 0 .. 3; the rows of the given streams are used (None = all).  Terms the kind does not use are stored as 0.
        Values are not judged."""
        B = self.num_streams
        coef = torch.as_tensor(coef, dtype=torch.float64)
        kind_host = kind.detach().cpu() if torch.is_tensor(kind) else torch.as_tensor(np.asarray(kind))
        if tuple(coef.shape) != (B, 2, 6):
            raise ValueError('set_screen_calibration: coef must be [%d, 2, 6] (stream, axis, term), got %s' % (B, tuple(coef.shape)))
        if tuple(kind_host.shape) != (B,) or kind_host.dtype.is_floating_point or kind_host.dtype == torch.bool or \
                int(kind_host.min()) < 0 or int(kind_host.max()) > 3:
            raise ValueError('set_screen_calibration: kind must be %d integers in 0 .. 3 (none, offset, affine, quadratic)' % B)
        terms = torch.tensor([0, 1, 3, 6])[kind_host.long()]
        coef = coef.to(self.device) * (torch.arange(6)[None, :] < terms[:, None]).to(torch.float64)[:, None, :].to(self.device)
        m = self._device_mask(streams, 'set_screen_calibration')
        self._screen_coef.copy_(torch.where(m[:, None, None], coef, self._screen_coef))
        self._screen_kind.copy_(torch.where(m, kind_host.to(torch.uint8).to(self.device), self._screen_kind))
        self._screen_apply = True

    def clear_screen_calibration(self, streams=None):
        """Forget the maps of the given streams (None = all): they get the uncorrected bits again.  The sample store stays."""
        self._zero_where(self._device_mask(streams, 'clear_screen_calibration'), self._screen_coef, self._screen_kind)
        if streams is None:
            self._screen_apply = False           # nothing left to apply: back to the launches of an EVEStream without a map

    def clear_screen_calibration_samples(self, streams=None):
        """Empty the screen map's sample store of the given streams (None = all), and their dropped counters."""
        if self._screen_store is None:
            self._stream_mask(streams, 'clear_screen_calibration_samples')
            return
        self._zero_where(self._device_mask(streams, 'clear_screen_calibration_samples'), self._screen_store.count, self._screen_store.dropped)

    def screen_calibration_counts(self):
        """-> (count, dropped), int32 [B] device tensors (fresh): the samples each stream holds, and those a full store
        (screen_calibration_capacity) turned away."""
        _, count, dropped = self._screen_samples()
        return count.clone(), dropped.clone()

    def screen_calibration_samples(self):
        """The sample store itself, float64 [B, C, 12] (fresh): rows 0 .. count - 1 of a stream in the order the frames came, in
        the layout of data.screen_calibration_samples / data.fit_screen_map."""
        return self._screen_samples()[0].clone()

    def _check_screen_calibration(self, chunk, B, Tc):
        """step()'s screen calibration keys, and what an applying step needs, checked before anything is launched or captured."""
        keys = ('inv_camera_transformation', 'pixels_per_millimeter')
        if self._screen_apply or chunk.get('screen_calibration_target') is None:      # applying: the corrected point's PoG_cm and g too
            keys += ('millimeters_per_pixel', 'camera_transformation')
        self._check_collecting(chunk, B, Tc, 'screen_calibration', self._screen_apply, self._screen_samples,
                               [(key, 'the screen geometry (%s)' % key) for key in keys],
                               ('left_o', 'the eyes\' origins o (left_o, right_o, or a pose form) in the chunk'))

    # ------------------------------------------------------------------ gaze events
    def _event_buffers(self):
        B, F = self.num_streams, self.fixation_capacity
        return self._group('_events', StageBuffers, ((B, 32), torch.float64), ((B, F, 8), torch.float64), ((B,), torch.int32), ((B,), torch.int32))

    def _closing_spec(self):
        from .data import GazeEventSpec
        return self._events_spec if self._events_spec is not None else GazeEventSpec()

    def fixations(self, streams=None, include_open=False):
        """The completed fixations of the given streams (None = all; indices or a bool mask), one numpy float64 [n, 8] array per
        stream in index order, rows (id, t_start, t_last, n samples, centroid x, centroid y, rms_px, 0) in the order they closed;
        times in the clock of the steps (frame_time, or frames / fps since the stream's last reset), pixels of the source PoG.  This
        call waits for the device.  include_open appends the fixation still running, as it stands, where it has lasted the last
        events step's min_fixation_s."""
        m = self._stream_mask(streams, 'fixations')
        state, store, count, _ = (t.cpu().numpy() for t in self._event_buffers())
        min_fix = self._closing_spec().min_fixation_s
        out = []
        for b in np.flatnonzero(m):
            rows = store[b, :min(max(int(count[b]), 0), self.fixation_capacity)].copy()
            r = state[b]
            if include_open and r[12] != 0 and r[22] - r[21] >= min_fix:
                n, mx, my = r[17], r[18] / r[17], r[19] / r[17]
                var = r[20] / n - (mx * mx + my * my)
                rows = np.concatenate([rows, np.array([[r[13], r[21], r[22], n, r[15] + mx, r[16] + my, np.sqrt(var) if var > 0 else 0.0, 0.0]])])
            out.append(rows)
        return out

    def fixation_counts(self):
        """-> (count, dropped), int32 [B] device tensors (fresh): the completed fixations each stream's store holds, and those a
        full store (fixation_capacity) turned away."""
        _, _, count, dropped = self._event_buffers()
        return count.clone(), dropped.clone()

    def clear_fixations(self, streams=None):
        """Empty the fixation store of the given streams (None = all) and their dropped counters.  The running fixation and the
        filter are state, not store: reset() ends them."""
        m = self._device_mask(streams, 'clear_fixations')
        buffers = self._event_buffers()
        self._zero_where(m, buffers.count, buffers.dropped)

    def flush_fixations(self, streams=None):
        """Close the open fixations of the given streams (None = all) on the device, as the end of a recording does: one
        eve_gaze_events launch with no frames.  A fixation that has lasted the last events step's min_fixation_s goes to the store."""
        flush = self._device_mask(streams, 'flush_fixations').to(torch.int32)
        state, store, count, dropped = self._event_buffers()
        default_kernels().gaze_events(None, None, None, None, self._closing_spec(), state, store, count, dropped, flush=flush)

    def get_event_state(self):
        """The gaze events' carried state, float64 [B, 32] (fresh; include/eve_hip.h eve_gaze_events has the layout): the filter, the
        last sample, the running fixation, the frame and id counters.  Resets not yet applied by a step are not reflected.
        get_state() / set_state() do not hold it."""
        return self._event_buffers()[0].clone()

    def set_event_state(self, state):
        """Load a state in get_event_state()'s layout, [B, 32] (converted to float64)."""
        state = torch.as_tensor(state, dtype=torch.float64).to(self.device)
        if tuple(state.shape) != (self.num_streams, 32):
            raise ValueError('set_event_state: state must be [%d, 32], got %s' % (self.num_streams, tuple(state.shape)))
        self._event_buffers()[0].copy_(state)
        self._saccades_stale = self._saccades is not None      # (the saccade row no longer follows this chain)
        self._pursuits_stale = self._pursuits is not None      # (nor does the pursuit row)

    def _output_stage(self):
        """'final' with a RefineNet, else 'initial': the stage whose point of gaze PoG_px_<out> is the step's output -- what the
        screen-space map corrects and what events and history take for a source of None."""
        return 'final' if self.model.refine_net is not None else 'initial'

    def _check_events(self, chunk, spec, B, Tc):
        """step()'s `events` checked against the chunk and the model -> what _predict_sequence needs beside the buffers.  Every
        refusal is a ValueError raised before anything is launched or captured."""
        from .data import GazeEventSpec
        if not isinstance(spec, GazeEventSpec):
            raise ValueError('step: events must be an eve_amd.GazeEventSpec, got %s' % type(spec).__name__)
        source = spec.source if spec.source is not None else 'PoG_px_' + self._output_stage()
        if source == 'PoG_px_final' and self.model.refine_net is None:
            raise ValueError('step: events filters PoG_px_final, which RefineNet produces, and the model has no RefineNet')
        for key in ('inv_camera_transformation', 'pixels_per_millimeter'):
            if key not in chunk:
                raise ValueError('step: events needs %s in the chunk: the gaze velocity is an angle at the eye' % key)
        if 'left_o' not in chunk and not has_pose_form(chunk):
            raise ValueError('step: events needs the eyes\' origins (left_o, right_o, or a pose form) in the chunk')
        ft = chunk.get('frame_time')
        if ft is None and spec.fps is None:
            raise ValueError('step: events needs frame_time in the chunk (float64 [B, Tc] seconds) or a spec with fps')
        if ft is not None:
            self._check_chunk_tensor('frame_time', ft, (torch.float64,), (B, Tc))
        self._event_buffers()                    # allocated here, before any capture
        return {'spec': spec, 'source': source}

    # ------------------------------------------------------------------ saccades
    def _saccade_buffers(self):
        B, S = self.num_streams, self.saccade_capacity
        return self._group('_saccades', SaccadeBuffers, ((B, 32), torch.float64), ((B, 16), torch.float64), ((B, S, 16), torch.float64),
                           ((B,), torch.int32), ((B,), torch.int32))

    def _saccade_launch_spec(self):
        from .data import SaccadeSpec
        return self._saccades_spec if self._saccades_spec is not None else SaccadeSpec()

    def _reset_saccade_rows(self, flags):
        """One eve_gaze_saccades launch with no frames: the flagged streams' open saccades are aborted and their rows start afresh."""
        default_kernels().gaze_saccades(None, None, None, None, None, None, None, self._saccade_launch_spec(), *self._saccade_buffers(),
                                        reset=flags)

    def saccades(self, streams=None):
        """The accepted saccades of the given streams (None = all; indices or a bool mask), one numpy float64 [n, 16] array per stream
        in index order, rows (id, t_onset, t_landing, n saccade frames, x0, y0, x1, y1, amplitude_deg, peak_deg_s, mean_deg_s,
        prev_fixation_id, next_fixation_id, missing, 0, 0) in the order they landed; times in the clock of the steps, pixels of the
        point the velocity is from.  The fixation ids are the events stage's: a fixation that never reached min_fixation_s is in no
        fixation store, and still has the id a row links to.  This call waits for the device."""
        m = self._stream_mask(streams, 'saccades')
        _, _, store, count, _ = (t.cpu().numpy() for t in self._saccade_buffers())
        return [store[b, :min(max(int(count[b]), 0), self.saccade_capacity)].copy() for b in np.flatnonzero(m)]

    def saccade_counts(self):
        """-> (count, dropped), int32 [B] device tensors (fresh): the accepted saccades each stream's store holds, and those a full
        store (saccade_capacity) turned away."""
        buffers = self._saccade_buffers()
        return buffers.count.clone(), buffers.dropped.clone()

    def saccade_table(self):
        """The tallies, float64 [B, 16] (fresh): accepted, sum_amp, sum_amp2, sum_peak, sum_amp_peak, sum_dur, sum_amp_dur, max_amp,
        max_peak, aborted, small, short, long, interrupted, 0, 0 (data.SACCADE_TABLE) -- degrees, degrees / second and seconds;
        data.main_sequence() fits the main sequence from them."""
        return self._saccade_buffers().table.clone()

    def clear_saccades(self, streams=None, table=False):
        """Empty the saccade store of the given streams (None = all) and their dropped counters; with table=True their tallies too.
        The open saccade is state, not store: reset() ends it."""
        m = self._device_mask(streams, 'clear_saccades')
        buffers = self._saccade_buffers()
        self._zero_where(m, buffers.count, buffers.dropped, *((buffers.table,) if table else ()))

    def get_saccade_state(self):
        """The saccade stage's carried state, float64 [B, 32] (fresh; include/eve_hip.h eve_gaze_saccades has the layout): the carried
        previous sample, the open saccade, the id counter.  Resets not yet applied by a step are not reflected.  get_state() /
        set_state() do not hold it."""
        return self._saccade_buffers().state.clone()

    def set_saccade_state(self, state):
        """Load a state in get_saccade_state()'s layout, [B, 32] (converted to float64), e.g. beside set_event_state() to resume a
        recording: the row is then taken to be in step with the events' row."""
        state = torch.as_tensor(state, dtype=torch.float64).to(self.device)
        if tuple(state.shape) != (self.num_streams, 32):
            raise ValueError('set_saccade_state: state must be [%d, 32], got %s' % (self.num_streams, tuple(state.shape)))
        self._saccade_buffers().state.copy_(state)
        self._saccades_stale = False

    def _check_saccades(self, spec, events):
        """step()'s `saccades` checked -> the stage's plan.  Every refusal is a ValueError raised before anything is launched or
        captured."""
        from .data import SaccadeSpec
        if not isinstance(spec, SaccadeSpec):
            raise ValueError('step: saccades must be an eve_amd.SaccadeSpec, got %s' % type(spec).__name__)
        if events is None:
            raise ValueError('step: saccades cuts the events stage\'s labels into saccades: pass events= in the same step')
        self._saccade_buffers()                  # allocated here, before any capture
        return {'spec': spec}

    # ------------------------------------------------------------------ smooth pursuit
    def _pursuit_buffers(self):
        B, S = self.num_streams, self.pursuit_capacity
        return self._group('_pursuits', PursuitBuffers, ((B, 320), torch.float64), ((B, 16), torch.float64), ((B, S, 20), torch.float64),
                           ((B,), torch.int32), ((B,), torch.int32))

    def _pursuit_launch_spec(self):
        from .data import PursuitSpec
        return self._pursuits_spec if self._pursuits_spec is not None else PursuitSpec()

    def _reset_pursuit_rows(self, flags):
        """One eve_gaze_pursuits launch with no frames: the flagged streams' open episodes are aborted and their rows start afresh."""
        default_kernels().gaze_pursuits(None, None, None, None, None, None, None, self._pursuit_launch_spec(), *self._pursuit_buffers(),
                                        reset=flags)

    def pursuits(self, streams=None):
        """The accepted pursuit episodes of the given streams (None = all; indices or a bool mask), one numpy float64 [n, 20] array per
        stream in index order, rows (id, t_onset, t_end, n pursuit frames, x0, y0, x1, y1, amplitude_deg, direction_deg (screen axes, y
        down), mean_deg_s, peak_deg_s, path_deg, fixation_id, missing, gain_n, mean_gain, mean_error_px, 0, 0: data.PURSUIT_COLUMNS) in
        the order they ended; times in the clock of the steps, pixels of the point the velocity is from.  fixation_id is the events
        stage's id of the "fixation" the episode lies in, so a consumer can discount that fixation; mean_gain and mean_error_px are NaN
        where no sample had a target.  This call waits for the device."""
        m = self._stream_mask(streams, 'pursuits')
        _, _, store, count, _ = (t.cpu().numpy() for t in self._pursuit_buffers())
        return [store[b, :min(max(int(count[b]), 0), self.pursuit_capacity)].copy() for b in np.flatnonzero(m)]

    def pursuit_counts(self):
        """-> (count, dropped), int32 [B] device tensors (fresh): the accepted episodes each stream's store holds, and those a full
        store (pursuit_capacity) turned away."""
        buffers = self._pursuit_buffers()
        return buffers.count.clone(), buffers.dropped.clone()

    def pursuit_table(self):
        """The tallies, float64 [B, 16] (fresh): accepted, sum_dur, sum_amp, sum_path, sum_mean_v, max_peak, sum_gain, gain_n, aborted,
        small, short, interrupted, 0 ... (data.PURSUIT_TABLE) -- seconds, degrees and degrees / second; data.pursuit_summary() reads
        them."""
        return self._pursuit_buffers().table.clone()

    def clear_pursuits(self, streams=None, table=False):
        """Empty the pursuit store of the given streams (None = all) and their dropped counters; with table=True their tallies too.
        The open episode is state, not store: reset() ends it."""
        m = self._device_mask(streams, 'clear_pursuits')
        buffers = self._pursuit_buffers()
        self._zero_where(m, buffers.count, buffers.dropped, *((buffers.table,) if table else ()))

    def get_pursuit_state(self):
        """The pursuit stage's carried state, float64 [B, 320] (fresh; include/eve_hip.h eve_gaze_pursuits has the layout): the run's
        last samples, the open episode, the id counter.  Resets not yet applied by a step are not reflected.  get_state() /
        set_state() do not hold it."""
        return self._pursuit_buffers().state.clone()

    def set_pursuit_state(self, state):
        """Load a state in get_pursuit_state()'s layout, [B, 320] (converted to float64), e.g. beside set_event_state() to resume a
        recording: the row is then taken to be in step with the events' row."""
        state = torch.as_tensor(state, dtype=torch.float64).to(self.device)
        if tuple(state.shape) != (self.num_streams, 320):
            raise ValueError('set_pursuit_state: state must be [%d, 320], got %s' % (self.num_streams, tuple(state.shape)))
        self._pursuit_buffers().state.copy_(state)
        self._pursuits_stale = False

    def _check_pursuits(self, chunk, spec, events, B, Tc):
        """step()'s `pursuits` checked against the chunk -> the stage's plan.  Every refusal is a ValueError raised before anything is
        launched or captured."""
        from .data import PursuitSpec
        if not isinstance(spec, PursuitSpec):
            raise ValueError('step: pursuits must be an eve_amd.PursuitSpec, got %s' % type(spec).__name__)
        if events is None:
            raise ValueError('step: pursuits looks for smooth pursuit among the events stage\'s fixation frames: pass events= in the same step')
        target = chunk.get('pursuit_target')
        if target is not None:
            self._check_chunk_tensor('pursuit_target', target, (torch.float32,), (B, Tc, 2))
        self._pursuit_buffers()                  # allocated here, before any capture
        return {'spec': spec, 'target': target is not None}

    # ------------------------------------------------------------------ the gaze history
    def _history_entry(self, spec, P):
        """The carried map and time chain of spec.name, made at the first step that names it.  A map is tied to its spec."""
        e = self._history.get(spec.name)
        if e is not None and (e['spec'].key() != spec.key() or e['P'] != P):
            if not e['free']:
                raise ValueError('step: history: the map %r was accumulated under another spec (%r); clear_gaze_history(%r) first' % (
                    spec.name, e['spec'], spec.name))
            e = None
            self._graphs = {}                    # (graphs captured on the old buffers)
        if e is None:
            B, (MW, MH) = self.num_streams, P['size']
            e = self._history[spec.name] = {'spec': spec, 'P': P, 'state': torch.zeros((B, 8), dtype=torch.float64, device=self.device),
                                            'maps': torch.zeros((B, MH, MW), dtype=torch.float32, device=self.device), 'free': False}
        e['free'] = False
        return e

    def _history_named(self, name, where):
        if name not in self._history:
            raise ValueError('%s: no gaze history map named %r (known: %s)' % (where, name, ', '.join(sorted(self._history)) or 'none'))
        return self._history[name]

    def gaze_history(self, name='gaze_history'):
        """The carried map of the history spec of that name, float32 [B, MH, MW] (a copy): the map after every stream's last consumed
        frame.  Resets not yet applied by a step are not reflected."""
        return self._history_named(name, 'gaze_history')['maps'].clone()

    def clear_gaze_history(self, name=None, streams=None):
        """Zero the maps and the time chains of the given streams (None = all) of one history spec, or of all of them (name=None).
        Cleared for all streams, a name may be taken by another spec at the next step."""
        entries = list(self._history.values()) if name is None else [self._history_named(name, 'clear_gaze_history')]
        if streams is None:
            for e in entries:
                e['maps'].zero_(), e['state'].zero_()
                e['free'] = True
            return
        m = self._device_mask(streams, 'clear_gaze_history')
        for e in entries:
            self._zero_where(m, e['maps'], e['state'])

    def get_gaze_history_state(self):
        """The gaze history's carried state: {name: {'spec': the GazeHistorySpec, 'maps': float32 [B, MH, MW], 'rows': float64 [B, 8]
        (has_prev, t_prev, ticks, reserved; include/eve_hip.h eve_gaze_history_plan)}}, fresh tensors.  Resets not yet applied by a
        step are not reflected.  get_state() / set_state() do not hold it."""
        return {name: {'spec': e['spec'], 'maps': e['maps'].clone(), 'rows': e['state'].clone()} for name, e in self._history.items()}

    def set_gaze_history_state(self, state):
        """Load maps and time chains in get_gaze_history_state()'s layout, e.g. to resume a recording.  A name that is known must come
        with the spec its map was accumulated under (or be cleared first)."""
        from .data import GazeHistorySpec
        B = self.num_streams
        loaded = []
        for name, s_ in state.items():
            spec = s_.get('spec') if isinstance(s_, dict) else None
            if not isinstance(spec, GazeHistorySpec) or spec.name != name:
                raise ValueError('set_gaze_history_state: %r needs its GazeHistorySpec under \'spec\'' % (name,))
            P = spec.launch_params(self.model.config)
            MW, MH = P['size']
            maps = torch.as_tensor(s_['maps'], dtype=torch.float32).to(self.device)
            rows = torch.as_tensor(s_['rows'], dtype=torch.float64).to(self.device)
            if tuple(maps.shape) != (B, MH, MW) or tuple(rows.shape) != (B, 8):
                raise ValueError('set_gaze_history_state: %r must hold maps [%d, %d, %d] and rows [%d, 8], got %s and %s' % (
                    name, B, MH, MW, B, tuple(maps.shape), tuple(rows.shape)))
            loaded.append((spec, P, maps, rows))
        for spec, P, maps, rows in loaded:
            e = self._history_entry(spec, P)
            e['maps'].copy_(maps), e['state'].copy_(rows)

    def _check_history(self, chunk, history, events, masked, B, Tc):
        """step()'s `history` checked against the chunk, the model and the step's other stages -> the plans _predict_sequence needs,
        buffers included.  Every refusal is a ValueError raised before anything is launched or captured."""
        from .data import GAZE_EVENT_KEYS, GazeHistorySpec
        specs = list(history) if isinstance(history, (list, tuple)) else [history]
        if not 1 <= len(specs) <= 2 or not all(isinstance(s_, GazeHistorySpec) for s_ in specs):
            raise ValueError('step: history must be an eve_amd.GazeHistorySpec or a list of one or two of them, got %s' % (
                ', '.join(type(s_).__name__ for s_ in specs) or 'an empty list'))
        if len({s_.name for s_ in specs}) != len(specs):
            raise ValueError('step: history: two specs share the name %r' % (specs[0].name,))
        cfg, has_ref = self.model.config, self.model.refine_net is not None
        taken = set(getattr(self.model, 'PREDICTION_KEYS', ())) | set(GAZE_EVENT_KEYS) | {'valid', 'eye_valid', 'pose_valid', 'rendered', 'heatmap_final'}
        ft = chunk.get('frame_time')
        if ft is not None:
            self._check_chunk_tensor('frame_time', ft, (torch.float64,), (B, Tc))
        plans = []
        for spec in specs:
            if spec.name in taken or spec.name in chunk or any(spec.name == s_.name + '_frames' for s_ in specs):
                raise ValueError('step: history: the name %r is a key of the chunk or of the step\'s result already' % (spec.name,))
            source = spec.source if spec.source is not None else 'PoG_px_' + self._output_stage()
            if source in ('PoG_px_final', 'heatmap_final') and not has_ref:
                raise ValueError('step: history accumulates %s, which RefineNet produces, and the model has no RefineNet' % source)
            if source in ('PoG_px_filtered', 'fixation_px') and events is None:
                raise ValueError('step: history accumulates %s, which the events stage produces: pass events= in the same step' % source)
            P = spec.launch_params(cfg)
            if source == 'heatmap_final' and tuple(P['size']) != (int(cfg.gaze_heatmap_size[0]), int(cfg.gaze_heatmap_size[1])):
                raise ValueError('step: history accumulates heatmap_final, so its size %r must be the config\'s gaze_heatmap_size %r' % (
                    tuple(P['size']), tuple(cfg.gaze_heatmap_size)))
            if 'inv_camera_transformation' not in chunk:
                raise ValueError('step: history accumulates %s, and the point of gaze needs the camera geometry '
                                 '(inv_camera_transformation) in the chunk' % source)
            vk = spec.valid_key
            if vk is not None:
                entry = chunk.get(vk)
                known = (vk == 'fixating' and events is not None) or (vk == 'valid' and masked)
                if entry is None and not known:
                    raise ValueError('step: history: valid_key %r is neither in the chunk nor a [B, Tc] result of this step' % (vk,))
                if entry is not None:
                    self._check_chunk_tensor('history: valid_key %r' % (vk,), entry, (torch.bool, torch.uint8), (B, Tc), got=False)
            if ft is None and spec.fps is None:
                raise ValueError('step: history needs frame_time in the chunk (float64 [B, Tc] seconds) or a spec with fps')
            e = self._history.get(spec.name)
            if e is not None and not e['free'] and (e['spec'].key() != spec.key() or e['P'] != P):
                self._history_entry(spec, P)     # (raises: the map is tied to another spec)
            plans.append({'spec': spec, 'source': source, 'P': P})
        return plans

    def _history_buffers(self, plans):
        """The plans' carried buffers, made here: after every refusal of the step, before any capture."""
        for plan in plans:
            e = self._history_entry(plan['spec'], plan['P'])
            plan['state'], plan['maps'] = e['state'], e['maps']

    def _reset_idle_stages(self, events, gate, history, aoi=None, pupil=None, saccades=None, pursuits=None):
        """A reset before a step that does not run a stage which carries state (events, gate, history, aoi, pupil, saccades, pursuits: None
        or this step's plans): the stage's state of the flagged streams still ends."""
        flags = self._flags[:self.num_streams]
        k = default_kernels()
        if saccades is None and self._saccades is not None:
            self._reset_saccade_rows(flags)      # the open saccade is aborted and the row starts afresh: the launch with no frames
        if pursuits is None and self._pursuits is not None:
            self._reset_pursuit_rows(flags)      # likewise the open pursuit episode
        if events is None and self._events is not None:
            # the gaze events' state ends its fixation and starts afresh: the launch with no frames
            k.gaze_events(None, None, None, None, self._closing_spec(), *self._events, reset=flags)
        running = set() if history is None else {p['spec'].name for p in history}
        for name, e in self._history.items():
            if name not in running:              # that map and its time chain are cleared by the two launches with no frames
                coef, clear = k.gaze_history_plan(e['P'], tuple(self.model.config.actual_screen_size), e['state'], 0, reset=flags)
                k.gaze_history_update(e['P'], coef, clear, e['maps'])
        if gate is None and self._gate is not None:
            self._zero_where(flags != 0, self._gate.state)       # the gate's rows (its launch refuses T = 0)
        for name, e in self._aoi.items():
            if aoi is None or aoi['spec'].name != name:          # that spec's open visit closes and its row starts afresh: no frames
                k.gaze_aoi(None, None, e['spec'], *e['buffers'], reset=flags)
        for name, e in self._pupil.items():
            if pupil is None or pupil['spec'].name != name:      # that spec's open episode closes and its row starts afresh: no frames
                k.pupil_track(None, e['spec'], *e['buffers'], reset=flags)

    # ------------------------------------------------------------------ pupillometry
    def _pupil_entry(self, spec):
        """The carried buffers of spec.name, made at the first step that names it.  The tallies are tied to their spec."""
        from .data import pupil_buffers
        e = self._pupil.get(spec.name)
        if e is not None and e['spec'].key() != spec.key():
            if not e['free']:
                raise ValueError('step: pupil: the tallies of %r were accumulated under another spec (%r); clear_pupil(%r) first' % (
                    spec.name, e['spec'], spec.name))
            e = None
            self._graphs = {}                    # (graphs captured on the old buffers)
        if e is None:
            e = self._pupil[spec.name] = {'spec': spec, 'free': False,
                                          'buffers': PupilBuffers(*pupil_buffers(self.num_streams, self.episode_capacity, self.device))}
        e['free'] = False
        return e

    def _pupil_named(self, name, where):
        """The entry of that name; None: the only one there is."""
        if name is None and len(self._pupil) == 1:
            return next(iter(self._pupil.values()))
        if name not in self._pupil:
            raise ValueError('%s: no pupillometry named %r (known: %s)' % (where, name, ', '.join(sorted(self._pupil)) or 'none'))
        return self._pupil[name]

    def pupil_table(self, name=None):
        """The table of the PupilSpec of that name (None: the only one), float64 [B, 24] (a copy): 0 covered_s (the time between
        connected samples) and 1 lost_s (the part of it that bridges frames which were no samples); 2 binocular, 3 left-only and 4
        right-only samples (the samples are their sum); 5-7 the left eye's rejects for not finite / range / speed, 8-10 the right eye's;
        11 d0 (the first sample's size), 12 sum(mm - d0), 13 sum((mm - d0)^2), 14 min and 15 max of mm; 16 n, 17 x0, 18 y0, 19 sum(x - x0),
        20 sum(y - y0), 21 sum((x - x0)^2), 22 sum((x - x0)(y - y0)), 23 sum((y - y0)^2) of the pairs x = the low-passed luminance, y = the
        filtered size before the light correction.  Times are in the clock of the steps."""
        return self._pupil_named(name, 'pupil_table')['buffers'].table.clone()

    def pupil_episodes(self, streams=None, name=None):
        """The completed dilation / constriction episodes of the given streams (None = all; indices or a bool mask), one numpy float64
        [n, 8] array per stream in index order, rows (phase +1 / -1, t_start, t_end, d_start, d_end, peak |velocity| in mm/s, samples,
        the low-passed luminance at the start or 0) in the order they ended.  This call waits for the device.  An episode still
        running is not in the store: flush_pupil_episodes() closes it."""
        m = self._stream_mask(streams, 'pupil_episodes')
        buffers = self._pupil_named(name, 'pupil_episodes')['buffers']
        store, count = buffers.store.cpu().numpy(), buffers.count.cpu().numpy()
        return [store[b, :min(max(int(count[b]), 0), self.episode_capacity)].copy() for b in np.flatnonzero(m)]

    def pupil_episode_counts(self, name=None):
        """-> (count, dropped), int32 [B] device tensors (fresh): the episodes each stream's store holds, and those a full store
        (episode_capacity) turned away."""
        buffers = self._pupil_named(name, 'pupil_episode_counts')['buffers']
        return buffers.count.clone(), buffers.dropped.clone()

    def clear_pupil(self, name=None, streams=None):
        """Zero the table, the episode store's counters and the state row of the given streams (None = all) of one PupilSpec, or of all
        of them (name=None): those streams start afresh, an episode still running is forgotten (flush_pupil_episodes() first keeps
        it).  The light response stays (clear_pupil_light_response()).  Cleared for all streams, a name may be taken by another spec
        at the next step."""
        entries = list(self._pupil.values()) if name is None else [self._pupil_named(name, 'clear_pupil')]
        m = None if streams is None else self._device_mask(streams, 'clear_pupil')
        for e in entries:
            state, table, _, _, count, dropped = e['buffers']
            if m is None:
                for t in (state, table, count, dropped):
                    t.zero_()
                e['free'] = True
            else:
                self._zero_where(m, state, table, count, dropped)

    def flush_pupil_episodes(self, streams=None, name=None):
        """Close the open episodes of the given streams (None = all) on the device, as the end of a recording does: one eve_pupil_track
        launch with no frames per PupilSpec (name=None: every one)."""
        flush = self._device_mask(streams, 'flush_pupil_episodes').to(torch.int32)
        for e in (list(self._pupil.values()) if name is None else [self._pupil_named(name, 'flush_pupil_episodes')]):
            default_kernels().pupil_track(None, e['spec'], *e['buffers'], flush=flush)

    def set_pupil_light_response(self, gain, ref, streams=None, name=None):
        """Set the light response of the given streams (None = all): from the next step on mm = filtered size - gain * (Lf - ref), Lf the
        low-passed pupil_luminance.  gain (mm per unit of luminance) and ref: numbers, or [B] (one per stream of the EVEStream)."""
        e = self._pupil_named(name, 'set_pupil_light_response')
        m = self._device_mask(streams, 'set_pupil_light_response')
        B = self.num_streams
        row = torch.zeros((B, 4), dtype=torch.float64)
        for col, v in ((1, gain), (2, ref)):
            v = torch.as_tensor(v, dtype=torch.float64).detach().cpu()
            if v.dim() > 1 or (v.dim() == 1 and v.shape[0] != B) or not bool(torch.isfinite(v).all()):
                raise ValueError('set_pupil_light_response: gain and ref must be finite numbers or [%d], got %r' % (B, tuple(v.shape)))
            row[:, col] = v
        row[:, 0] = 1.0
        light = e['buffers'].light
        light.copy_(torch.where(m[:, None], self._pinned(row).to(self.device, non_blocking=True), light))

    def get_pupil_light_response(self, name=None):
        """-> float64 [B, 4] (a copy): rows (has_gain, gain, ref, 0)."""
        return self._pupil_named(name, 'get_pupil_light_response')['buffers'].light.clone()

    def clear_pupil_light_response(self, streams=None, name=None):
        """The given streams (None = all) go back to the uncorrected trace."""
        e = self._pupil_named(name, 'clear_pupil_light_response')
        self._zero_where(self._device_mask(streams, 'clear_pupil_light_response'), e['buffers'].light)

    def fit_pupil_light_response(self, streams=None, min_samples=30, name=None):
        """Fit the light response of the given streams (None = all) from the table's regression sums of (low-passed luminance, filtered
        size): gain = Sxy / Sxx, ref = x0 + Sx / n (the mean luminance, so the correction leaves the mean size alone).  A stream with
        fewer than min_samples pairs, or whose luminance did not move (Sxx == 0), keeps what it had.  A few float64 operations on
        the device; the host does not wait.  Collect with the response cleared: the sums are of the size BEFORE the correction."""
        if isinstance(min_samples, bool) or not isinstance(min_samples, (int, np.integer)) or min_samples < 2:
            raise ValueError('fit_pupil_light_response: min_samples must be an integer >= 2, got %r' % (min_samples,))
        e = self._pupil_named(name, 'fit_pupil_light_response')
        m = self._device_mask(streams, 'fit_pupil_light_response')
        table, light = e['buffers'].table, e['buffers'].light
        n, x0, sx, sxx, sxy = table[:, 16], table[:, 17], table[:, 19], table[:, 21], table[:, 22]
        ok = m & (n >= float(min_samples)) & (sxx > 0)
        one = torch.ones_like(n)
        fitted = torch.stack([one, sxy / torch.where(ok, sxx, one), x0 + sx / torch.where(ok, n, one), torch.zeros_like(n)], dim=1)
        light.copy_(torch.where(ok[:, None], fitted, light))

    def get_pupil_state(self):
        """What the pupillometry carries: {name: {'spec': the PupilSpec, 'state': float64 [B, 32] (include/eve_hip.h eve_pupil_track has
        the layout), 'table': float64 [B, 24], 'light': float64 [B, 4], 'episodes': float64 [B, episode_capacity, 8], 'count', 'dropped':
        int32 [B]}}, fresh tensors.  Resets not yet applied by a step are not reflected.  get_state() / set_state() do not hold it."""
        return {name: dict({'spec': e['spec']}, **{('episodes' if k_ == 'store' else k_): t.clone() for k_, t in e['buffers']._asdict().items()})
                for name, e in self._pupil.items()}

    def set_pupil_state(self, state):
        """Load what get_pupil_state() returned, e.g. to resume a recording.  A name that is known must come with the spec its tallies
        were accumulated under (or be cleared first)."""
        from .data import PUPIL_STATE, PUPIL_TABLE, PupilSpec
        B, V = self.num_streams, self.episode_capacity
        loaded = []
        for name, s_ in state.items():
            spec = s_.get('spec') if isinstance(s_, dict) else None
            if not isinstance(spec, PupilSpec) or spec.name != name:
                raise ValueError('set_pupil_state: %r needs its PupilSpec under \'spec\'' % (name,))
            tensors = []
            for key, dtype, shape in (('state', torch.float64, (B, PUPIL_STATE)), ('table', torch.float64, (B, PUPIL_TABLE)),
                                      ('light', torch.float64, (B, 4)), ('episodes', torch.float64, (B, V, 8)),
                                      ('count', torch.int32, (B,)), ('dropped', torch.int32, (B,))):
                t = torch.as_tensor(s_[key], dtype=dtype).to(self.device)
                if tuple(t.shape) != shape:
                    raise ValueError('set_pupil_state: %r: %s must be %s, got %s' % (name, key, list(shape), tuple(t.shape)))
                tensors.append(t)
            e = self._pupil.get(name)
            if e is not None and not e['free'] and e['spec'].key() != spec.key():
                self._pupil_entry(spec)          # (raises: the tallies are tied to another spec -- before anything is loaded)
            loaded.append((spec, tensors))
        for spec, tensors in loaded:
            for dst, src in zip(self._pupil_entry(spec)['buffers'], tensors):
                dst.copy_(src)

    def _check_pupil(self, chunk, spec, events, history, aoi, gate, B, Tc):
        """step()'s `pupil` checked against the chunk and the step's other stages -> what _predict_sequence needs beside the buffers.
        Every refusal is a ValueError raised before anything is launched or captured."""
        from .data import AOI_KEYS, EYE_GATE_KEYS, GAZE_EVENT_KEYS, PUPIL_KEYS, PupilSpec
        if not isinstance(spec, PupilSpec):
            raise ValueError('step: pupil must be an eve_amd.PupilSpec, got %s' % type(spec).__name__)
        taken = set(getattr(self.model, 'PREDICTION_KEYS', ())) | set(GAZE_EVENT_KEYS) | {'valid', 'eye_valid', 'pose_valid', 'rendered', 'heatmap_final'}
        if gate is not None:
            taken |= set(EYE_GATE_KEYS)
        for h in history or ():
            taken |= {h['spec'].name, h['spec'].name + '_frames'}
        if aoi is not None:
            taken |= {'%s_%s' % (aoi['spec'].name, k_) for k_ in AOI_KEYS}
        for key in PUPIL_KEYS:
            if '%s_%s' % (spec.name, key) in taken or '%s_%s' % (spec.name, key) in chunk:
                raise ValueError('step: pupil: the name %r gives %s_%s, which is a key of the chunk or of the step\'s result already' % (
                    spec.name, spec.name, key))
        if 'pupil_luminance' in chunk:
            self._check_chunk_tensor('pupil_luminance', chunk['pupil_luminance'], (torch.float32,), (B, Tc))
        if 'pupil_baseline' in chunk:
            self._check_chunk_tensor('pupil_baseline', chunk['pupil_baseline'], (torch.bool, torch.uint8), (B, Tc))
        ft = chunk.get('frame_time')
        if ft is None and spec.fps is None:
            raise ValueError('step: pupil needs frame_time in the chunk (float64 [B, Tc] seconds) or a spec with fps')
        if ft is not None:
            self._check_chunk_tensor('frame_time', ft, (torch.float64,), (B, Tc))
        e = self._pupil.get(spec.name)
        if e is not None and not e['free'] and e['spec'].key() != spec.key():
            self._pupil_entry(spec)              # (raises: the tallies are tied to another spec)
        return {'spec': spec}

    # ------------------------------------------------------------------ screen luminance
    def _check_luminance(self, chunk, spec, events, history, aoi, pupil, gate, masked, B, Tc):
        """step()'s `luminance` checked against the chunk, the model and the step's other stages -> what _predict_sequence needs: the
        capture's key, its layout and matrix, the discs' source, radii and scale, the response table on the device.  Every refusal is
        a ValueError raised before anything is launched or captured."""
        from .data import AOI_KEYS, EYE_GATE_KEYS, GAZE_EVENT_KEYS, PUPIL_KEYS, ScreenLuminanceSpec, capture_layout, surface_frames
        from .kernels import YUV_MATRICES
        from .refine_net import SCREEN_FRAME_KEYS, SCREEN_SURFACE_KEY, screen_frame_key
        if not isinstance(spec, ScreenLuminanceSpec):
            raise ValueError('step: luminance must be an eve_amd.ScreenLuminanceSpec, got %s' % type(spec).__name__)
        taken = set(getattr(self.model, 'PREDICTION_KEYS', ())) | set(GAZE_EVENT_KEYS) | {'valid', 'eye_valid', 'pose_valid', 'rendered', 'heatmap_final'}
        if gate is not None:
            taken |= set(EYE_GATE_KEYS)
        for h in history or ():
            taken |= {h['spec'].name, h['spec'].name + '_frames'}
        if aoi is not None:
            taken |= {'%s_%s' % (aoi['spec'].name, k_) for k_ in AOI_KEYS}
        if pupil is not None:
            taken |= {'%s_%s' % (pupil['spec'].name, k_) for k_ in PUPIL_KEYS}
        for key in spec.result_keys():
            if key in taken or key in chunk:
                raise ValueError('step: luminance: the name %r gives %s, which is a key of the chunk or of the step\'s result already' % (spec.name, key))
        cfg, ref = self.model.config, self.model.refine_net
        key = screen_frame_key(chunk)
        if key is None:
            raise ValueError('step: luminance reads the screen capture, and the chunk holds none (screen_frame, one of %s, or %s)' % (
                ', '.join(k_ for k_ in SCREEN_FRAME_KEYS if k_ != 'screen_frame'), SCREEN_SURFACE_KEY))
        frames = chunk[key]
        net_hw = (int(cfg.screen_size[1]), int(cfg.screen_size[0]))
        if key == 'screen_frame' and (not torch.is_tensor(frames) or frames.dtype != torch.uint8 or frames.dim() != 5 or
                                      frames.shape[4] not in (3, 4) or tuple(frames.shape[2:4]) == net_hw):
            raise ValueError('step: luminance needs a full-resolution uint8 capture [B, Tc, IH, IW, 3 | 4] to read; screen_frame is %s %s '
                             '(a float or %d x %d screen_frame is the network\'s input, not a capture)' % (
                                 getattr(frames, 'dtype', type(frames)), tuple(getattr(frames, 'shape', ())), net_hw[0], net_hw[1]))
        try:
            if key == SCREEN_SURFACE_KEY:
                layout = None if ref is None else ref.screen_layout
                if layout is None:
                    raise ValueError('%s needs RefineNet.screen_layout, a data.SurfaceLayout that says how the capture lies in memory' % key)
                surface_frames(frames, layout, 2, name=key)
            else:
                layout = capture_layout(frames, SCREEN_FRAME_KEYS[key], 2, name=key)
        except (TypeError, ValueError) as e:
            raise ValueError('step: luminance: %s' % e)
        if tuple(frames.shape[:2]) != (B, Tc) or frames.device != self.device or not frames.is_contiguous():
            raise ValueError('step: luminance: %s must be a contiguous [%d, %d, ...] tensor on %s, got %s on %s' % (
                key, B, Tc, self.device, tuple(frames.shape), frames.device))
        matrix = ref.yuv_matrix if ref is not None else 'bt601'
        if matrix not in YUV_MATRICES:
            raise ValueError('step: luminance: RefineNet.yuv_matrix must be one of %s, got %r' % (', '.join(YUV_MATRICES), matrix))
        if spec.to_pupil is not None and 'pupil_luminance' in chunk:
            raise ValueError('step: luminance: to_pupil makes the covariate the pupil stage\'s luminance, and the chunk brings pupil_luminance '
                             'too: drop one of them (to_pupil=None keeps the chunk\'s)')
        sx, sy = layout.width / float(cfg.actual_screen_size[0]), layout.height / float(cfg.actual_screen_size[1])
        source, radii = None, ()
        if spec.radii_px:
            source = spec.source if spec.source is not None else 'PoG_px_' + self._output_stage()
            if source == 'PoG_px_final' and ref is None:
                raise ValueError('step: luminance follows PoG_px_final, which RefineNet produces, and the model has no RefineNet')
            if source in ('PoG_px_filtered', 'fixation_px') and events is None:
                raise ValueError('step: luminance follows %s, which the events stage produces: pass events= in the same step' % source)
            if 'inv_camera_transformation' not in chunk:
                raise ValueError('step: luminance follows %s, and the point of gaze needs the camera geometry (inv_camera_transformation) '
                                 'in the chunk' % source)
            radii = spec.capture_radii(sx, 'step: luminance')
            vk = spec.valid_key
            if vk is not None:
                entry = chunk.get(vk)
                known = (vk == 'fixating' and events is not None) or (vk == 'valid' and masked)
                if entry is None and not known:
                    raise ValueError('step: luminance: valid_key %r is neither in the chunk nor a [B, Tc] result of this step' % (vk,))
                if entry is not None:
                    self._check_chunk_tensor('luminance: valid_key %r' % (vk,), entry, (torch.bool, torch.uint8), (B, Tc), got=False)
        table = self._luminance_tables.get(spec.key())
        if table is None:                        # made here, before any capture: a host-to-device copy
            table = self._luminance_tables[spec.key()] = spec.response_table().to(self.device)
        return {'spec': spec, 'key': key, 'layout': layout, 'matrix': matrix, 'source': source, 'radii': radii, 'sx': sx, 'sy': sy, 'table': table}

    # ------------------------------------------------------------------ areas of interest
    def _aoi_entry(self, spec):
        """The carried buffers of spec.name, made at the first step that names it.  The tallies are tied to their spec."""
        from .data import aoi_buffers
        e = self._aoi.get(spec.name)
        if e is not None and e['spec'].key() != spec.key():
            if not e['free']:
                raise ValueError('step: aoi: the tallies of %r were accumulated under another spec (%r); clear_aoi(%r) first' % (
                    spec.name, e['spec'], spec.name))
            e = None
            self._graphs = {}                    # (graphs captured on the old buffers)
        if e is None:
            e = self._aoi[spec.name] = {'spec': spec, 'free': False,
                                        'buffers': AoiBuffers(*aoi_buffers(self.num_streams, spec.num_aois, self.visit_capacity, self.device))}
        e['free'] = False
        return e

    def _aoi_named(self, name, where):
        """The entry of that name; None: the only one there is."""
        if name is None and len(self._aoi) == 1:
            return next(iter(self._aoi.values()))
        if name not in self._aoi:
            raise ValueError('%s: no areas of interest named %r (known: %s)' % (where, name, ', '.join(sorted(self._aoi)) or 'none'))
        return self._aoi[name]

    def aoi_table(self, name=None):
        """The dwell table of the AoiSpec of that name (None: the only one), float64 [B, A + 1, 8] (a copy): per stream and AOI the row
        (dwell_s, samples, visits, t_first_entry, t_last, fixations, t_first_fixation, 0); row A is "no AOI".  dwell_s is the time between
        connected samples inside the AOI, times in the clock of the steps (frame_time, or frames / fps since the stream's last reset)."""
        return self._aoi_named(name, 'aoi_table')['buffers'].table.clone()

    def aoi_transitions(self, name=None):
        """The transition matrix of the AoiSpec of that name (None: the only one), int32 [B, A + 1, A] (a copy): [from][to] counts the
        visits to `to` that followed a visit to `from`; row A is the first visit since a reset, the diagonal counts revisits (the same
        AOI after time outside all of them, or after a gap).  Every column sums to the AOI's visits."""
        return self._aoi_named(name, 'aoi_transitions')['buffers'].trans.clone()

    def aoi_visits(self, streams=None, name=None):
        """The completed visits of the given streams (None = all; indices or a bool mask), one numpy float64 [n, 8] array per stream in
        index order, rows (aoi, t_enter, t_last, samples, fixations, visit_index, 0, 0) in the order they ended.  This call waits for
        the device.  A visit still running is not in the store: flush_aoi_visits() closes it."""
        m = self._stream_mask(streams, 'aoi_visits')
        buffers = self._aoi_named(name, 'aoi_visits')['buffers']
        store, count = buffers.visits.cpu().numpy(), buffers.count.cpu().numpy()
        return [store[b, :min(max(int(count[b]), 0), self.visit_capacity)].copy() for b in np.flatnonzero(m)]

    def aoi_visit_counts(self, name=None):
        """-> (count, dropped), int32 [B] device tensors (fresh): the completed visits each stream's store holds, and those a full
        store (visit_capacity) turned away."""
        buffers = self._aoi_named(name, 'aoi_visit_counts')['buffers']
        return buffers.count.clone(), buffers.dropped.clone()

    def clear_aoi(self, name=None, streams=None):
        """Zero the dwell table, the transitions, the visit store's counters and the state row of the given streams (None = all) of one
        AoiSpec, or of all of them (name=None): those streams start afresh, a visit still running is forgotten (flush_aoi_visits()
        first keeps it).  Cleared for all streams, a name may be taken by another spec at the next step."""
        entries = list(self._aoi.values()) if name is None else [self._aoi_named(name, 'clear_aoi')]
        m = None if streams is None else self._device_mask(streams, 'clear_aoi')
        for e in entries:
            state, table, trans, _, count, dropped = e['buffers']
            if m is None:
                for t in (state, table, trans, count, dropped):
                    t.zero_()
                e['free'] = True
            else:
                self._zero_where(m, state, table, trans, count, dropped)

    def flush_aoi_visits(self, streams=None, name=None):
        """Close the open visits of the given streams (None = all) on the device, as the end of a recording does: one eve_gaze_aoi launch
        with no frames per AoiSpec (name=None: every one)."""
        flush = self._device_mask(streams, 'flush_aoi_visits').to(torch.int32)
        for e in (list(self._aoi.values()) if name is None else [self._aoi_named(name, 'flush_aoi_visits')]):
            default_kernels().gaze_aoi(None, None, e['spec'], *e['buffers'], flush=flush)

    def get_aoi_state(self):
        """What the areas of interest carry: {name: {'spec': the AoiSpec, 'state': float64 [B, 16] (include/eve_hip.h eve_gaze_aoi has the
        layout), 'table': float64 [B, A + 1, 8], 'transitions': int32 [B, A + 1, A], 'visits': float64 [B, visit_capacity, 8], 'count',
        'dropped': int32 [B]}}, fresh tensors.  Resets not yet applied by a step are not reflected.  get_state() / set_state() do not
        hold it."""
        return {name: dict({'spec': e['spec']}, **{('transitions' if k_ == 'trans' else k_): t.clone() for k_, t in e['buffers']._asdict().items()})
                for name, e in self._aoi.items()}

    def set_aoi_state(self, state):
        """Load what get_aoi_state() returned, e.g. to resume a recording.  A name that is known must come with the spec its tallies were
        accumulated under (or be cleared first)."""
        from .data import AoiSpec
        B, V = self.num_streams, self.visit_capacity
        loaded = []
        for name, s_ in state.items():
            spec = s_.get('spec') if isinstance(s_, dict) else None
            if not isinstance(spec, AoiSpec) or spec.name != name:
                raise ValueError('set_aoi_state: %r needs its AoiSpec under \'spec\'' % (name,))
            A = spec.num_aois
            tensors = []
            for key, dtype, shape in (('state', torch.float64, (B, 16)), ('table', torch.float64, (B, A + 1, 8)),
                                      ('transitions', torch.int32, (B, A + 1, A)), ('visits', torch.float64, (B, V, 8)),
                                      ('count', torch.int32, (B,)), ('dropped', torch.int32, (B,))):
                t = torch.as_tensor(s_[key], dtype=dtype).to(self.device)
                if tuple(t.shape) != shape:
                    raise ValueError('set_aoi_state: %r: %s must be %s, got %s' % (name, key, list(shape), tuple(t.shape)))
                tensors.append(t)
            e = self._aoi.get(name)
            if e is not None and not e['free'] and e['spec'].key() != spec.key():
                self._aoi_entry(spec)            # (raises: the tallies are tied to another spec -- before anything is loaded)
            loaded.append((spec, tensors))
        for spec, tensors in loaded:
            for dst, src in zip(self._aoi_entry(spec)['buffers'], tensors):
                dst.copy_(src)

    def _check_aoi(self, chunk, spec, events, history, masked, B, Tc):
        """step()'s `aoi` checked against the chunk, the model and the step's other stages -> what _predict_sequence needs beside the
        buffers.  Every refusal is a ValueError raised before anything is launched or captured."""
        from .data import AOI_KEYS, AOI_ROW, GAZE_EVENT_KEYS, AoiSpec
        if not isinstance(spec, AoiSpec):
            raise ValueError('step: aoi must be an eve_amd.AoiSpec, got %s' % type(spec).__name__)
        A = spec.num_aois
        taken = set(getattr(self.model, 'PREDICTION_KEYS', ())) | set(GAZE_EVENT_KEYS) | {'valid', 'eye_valid', 'pose_valid', 'rendered', 'heatmap_final'}
        for h in history or ():
            taken |= {h['spec'].name, h['spec'].name + '_frames'}
        for key in AOI_KEYS:
            if '%s_%s' % (spec.name, key) in taken or '%s_%s' % (spec.name, key) in chunk:
                raise ValueError('step: aoi: the name %r gives %s_%s, which is a key of the chunk or of the step\'s result already' % (
                    spec.name, spec.name, key))
        shapes = chunk.get('aoi_shapes')
        if shapes is None:
            raise ValueError('step: aoi needs aoi_shapes in the chunk: float32 [%d, %d, %d] or [%d, %d, %d, %d] (data.aoi_shapes)' % (
                B, A, AOI_ROW, B, Tc, A, AOI_ROW))
        if torch.is_tensor(shapes) and shapes.dim() == 4:
            self._check_chunk_tensor('aoi_shapes', shapes, (torch.float32,), (B, Tc, A, AOI_ROW))
        else:
            self._check_chunk_tensor('aoi_shapes', shapes, (torch.float32,), (B, A, AOI_ROW))
        source = spec.source if spec.source is not None else 'PoG_px_' + self._output_stage()
        if source == 'PoG_px_final' and self.model.refine_net is None:
            raise ValueError('step: aoi tests PoG_px_final, which RefineNet produces, and the model has no RefineNet')
        if source in ('PoG_px_filtered', 'fixation_px') and events is None:
            raise ValueError('step: aoi tests %s, which the events stage produces: pass events= in the same step' % source)
        if 'inv_camera_transformation' not in chunk:
            raise ValueError('step: aoi tests %s, and the point of gaze needs the camera geometry (inv_camera_transformation) in the '
                             'chunk' % source)
        vk = spec.valid_key
        if vk is not None:
            entry = chunk.get(vk)
            known = (vk == 'fixating' and events is not None) or (vk == 'valid' and masked)
            if entry is None and not known:
                raise ValueError('step: aoi: valid_key %r is neither in the chunk nor a [B, Tc] result of this step' % (vk,))
            if entry is not None:
                self._check_chunk_tensor('aoi: valid_key %r' % (vk,), entry, (torch.bool, torch.uint8), (B, Tc), got=False)
        if spec.use_fixations and events is None:
            raise ValueError('step: aoi: use_fixations=True counts the events stage\'s fixations: pass events= in the same step')
        ft = chunk.get('frame_time')
        if ft is None and spec.fps is None:
            raise ValueError('step: aoi needs frame_time in the chunk (float64 [B, Tc] seconds) or a spec with fps')
        if ft is not None:
            self._check_chunk_tensor('frame_time', ft, (torch.float64,), (B, Tc))
        e = self._aoi.get(spec.name)
        if e is not None and not e['free'] and e['spec'].key() != spec.key():
            self._aoi_entry(spec)                # (raises: the tallies are tied to another spec)
        return {'spec': spec, 'source': source, 'use_fixations': events is not None if spec.use_fixations is None else spec.use_fixations}

    # ------------------------------------------------------------------ the eye gate
    def _gate_buffers(self):
        B, C = self.num_streams, self.blink_capacity
        return self._group('_gate', StageBuffers, ((B, 2, 8), torch.float64), ((B, C, 4), torch.float64), ((B,), torch.int32), ((B,), torch.int32))

    def blinks(self, streams=None):
        """The completed blinks of the given streams (None = all; indices or a bool mask), one numpy float64 [n, 4] array per stream
        in index order, rows (eye: 0 left, 1 right; the tick of the first closed frame; the tick of the last one; the minimum
        openness) in the order they ended; a tick counts the stream's delivered frames since its last reset.  This call waits for
        the device.  A closure still running, one that a reset() cut short and one longer than max_closed_frames are not blinks."""
        m = self._stream_mask(streams, 'blinks')
        _, store, count, _ = (t.cpu().numpy() for t in self._gate_buffers())
        return [store[b, :min(max(int(count[b]), 0), self.blink_capacity)].copy() for b in np.flatnonzero(m)]

    def blink_counts(self):
        """-> (count, dropped), int32 [B] device tensors (fresh): the completed blinks each stream's store holds, and those a full
        store (blink_capacity) turned away."""
        _, _, count, dropped = self._gate_buffers()
        return count.clone(), dropped.clone()

    def clear_blinks(self, streams=None):
        """Empty the blink store of the given streams (None = all) and their dropped counters.  The running closure, the baseline
        and the hold-off are state, not store: reset() ends them."""
        m = self._device_mask(streams, 'clear_blinks')
        buffers = self._gate_buffers()
        self._zero_where(m, buffers.count, buffers.dropped)

    def get_gate_state(self):
        """The eye gate's carried state, float64 [B, 2, 8] (fresh; include/eve_hip.h eve_eye_gate has the layout): per stream and eye
        the baseline, the running closure, the hold-off and the stream's frame count.  Resets not yet applied by a step are not
        reflected.  get_state() / set_state() do not hold it."""
        return self._gate_buffers()[0].clone()

    def set_gate_state(self, state):
        """Load a state in get_gate_state()'s layout, [B, 2, 8] (converted to float64)."""
        state = torch.as_tensor(state, dtype=torch.float64).to(self.device)
        if tuple(state.shape) != (self.num_streams, 2, 8):
            raise ValueError('set_gate_state: state must be [%d, 2, 8], got %s' % (self.num_streams, tuple(state.shape)))
        self._gate_buffers()[0].copy_(state)

    def _check_gate(self, chunk, spec, B, Tc):
        """step()'s `gate` checked against the chunk and the model -> what _predict_sequence needs beside the buffers.  Every
        refusal is a ValueError raised before anything is launched or captured."""
        from .data import EYE_CONTOURS_KEY, EyeGateSpec, check_eye_contours
        from .eye_net import EYE_FRAME_KEYS, EYE_SURFACE_KEY, FACE_LANDMARKS_RAW_KEY, camera_frame_key
        from .kernels import pixel_format_shape
        if not isinstance(spec, EyeGateSpec):
            raise ValueError('step: gate must be an eve_amd.EyeGateSpec, got %s' % type(spec).__name__)
        frame_key, lm_key = camera_frame_key(chunk), face_landmarks_key(chunk)
        if frame_key is None and (spec.min_coverage is not None or spec.head_angles):
            raise ValueError('step: gate: %s needs a camera form (a camera frame with warps, eye_pose or face_landmarks): pre-cut patches '
                             'have no warp and no derived head angles to test' % ('min_coverage' if spec.min_coverage is not None else
                                                                                   'head_pitch / head_yaw_left / head_yaw_right'))
        if spec.max_reproj_px is not None and lm_key is None:
            raise ValueError('step: gate: max_reproj_px tests face_reproj_rms, which the face-landmark form produces')
        if spec.min_inliers is not None and (lm_key is None or (lm_key != FACE_LANDMARKS_RAW_KEY and self.model.eye_net.face_huber_px is None)):
            raise ValueError('step: gate: min_inliers tests face_inliers, which the face-landmark form produces with eye_net.face_huber_px '
                             'or face_landmarks_raw')
        if spec.blink is not None and EYE_CONTOURS_KEY not in chunk:
            raise ValueError('step: gate: blink needs %s in the chunk (float32 [B, Tc, 2, 6, 2 | 3])' % EYE_CONTOURS_KEY)
        if EYE_CONTOURS_KEY in chunk:
            check_eye_contours(chunk[EYE_CONTOURS_KEY], B, Tc, self.device, 'step: gate')
        frame_size = None
        if spec.min_coverage is not None:
            if frame_key == EYE_SURFACE_KEY:
                layout = self.model.eye_net.camera_layout
                if layout is None:
                    raise ValueError('step: gate: min_coverage needs the frame size, and %s comes without eye_net.camera_layout' % frame_key)
                frame_size = (int(layout.width), int(layout.height))
            else:
                try:
                    IH, IW, _ = pixel_format_shape(chunk[frame_key], EYE_FRAME_KEYS[frame_key], lead=2, name=frame_key)
                except TypeError as e:
                    raise ValueError('step: gate: %s' % e)
                frame_size = (int(IW), int(IH))
        self._gate_buffers()                     # allocated here, before any capture
        return {'spec': spec, 'frame_size': frame_size}

    def get_state(self):
        """The carried states in the reference layout (fresh tensors): {left,right}_eye_rnn_states_<i> [B, H] float32 ((h, c) for
        LSTM) and refinenet_rnn_states_<i> [B, C, 5, 8] float32 ((h, c) for CLSTM).  Resets not yet applied by a step are not
        reflected."""
        B = self.num_streams
        st = {}
        for i, buf in enumerate(self._eye):
            for si, side in enumerate(('left', 'right')):
                cut = lambda t: t[si * B:(si + 1) * B].clone()
                st['%s_eye_rnn_states_%d' % (side, i)] = tuple(cut(t) for t in buf) if isinstance(buf, tuple) else cut(buf)
        if self._ref:
            C = self.model.config.refine_net_num_features
            ref = lambda t: t[..., :C].permute(0, 3, 1, 2).float().contiguous()
            for i, buf in enumerate(self._ref):
                st['refinenet_rnn_states_%d' % i] = tuple(ref(t) for t in buf) if isinstance(buf, tuple) else ref(buf)
        return st

    def set_state(self, state):
        """Load states in get_state()'s layout (every key it returns); cancels resets requested since the last step."""
        B = self.num_streams
        for i, buf in enumerate(self._eye):
            for si, side in enumerate(('left', 'right')):
                v = state['%s_eye_rnn_states_%d' % (side, i)]
                for dst, src in (zip(buf, v) if isinstance(buf, tuple) else ((buf, v),)):
                    dst[si * B:(si + 1) * B].copy_(src)
        if self._ref:
            C = self.model.config.refine_net_num_features
            for i, buf in enumerate(self._ref):
                v = state['refinenet_rnn_states_%d' % i]
                for dst, src in (zip(buf, v) if isinstance(buf, tuple) else ((buf, v),)):
                    if tuple(src.shape) != (B, C, dst.shape[1], dst.shape[2]):
                        raise ValueError('set_state: refinenet_rnn_states_%d must be [%d, %d, %d, %d]' % (i, B, C, dst.shape[1], dst.shape[2]))
                    dst[..., :C].copy_(src.permute(0, 2, 3, 1))
        self._pending = None

    def get_head_pose(self):
        """The head pose the face-landmark form carries from one step to the next (fresh tensors): R float64 [B, 3, 3], t float64
        [B, 3] and has_pose bool [B] -- False where the stream's next frame starts cold (no frame yet, a reset applied, a last
        frame without a solution).  Resets not yet applied by a step are not reflected.  get_state() / set_state() do not hold
        it: a resumed recording re-acquires the pose from a cold start within one frame."""
        s = self._face_pose
        return s[:, :9].reshape(-1, 3, 3).clone(), s[:, 9:12].clone(), s[:, 12] != 0

    def set_head_pose(self, R, t, has_pose=True):
        """Load a carried head pose in get_head_pose()'s layout: R [B, 3, 3], t [B, 3] (converted to float64), has_pose a bool or B
        of them.  The next face-landmark step starts stream b from (R[b], t[b]) where has_pose[b], cold elsewhere."""
        B = self.num_streams
        R = torch.as_tensor(R, dtype=torch.float64).to(self.device)
        t = torch.as_tensor(t, dtype=torch.float64).to(self.device)
        if tuple(R.shape) != (B, 3, 3) or tuple(t.shape) != (B, 3):
            raise ValueError('set_head_pose: R must be [%d, 3, 3] and t [%d, 3], got %s and %s' % (B, B, tuple(R.shape), tuple(t.shape)))
        has = torch.as_tensor(has_pose, dtype=torch.bool).to(self.device).expand(B)
        self._face_pose.copy_(torch.cat([R.reshape(B, 9), t, has.to(torch.float64)[:, None]], dim=1))

    # ------------------------------------------------------------------ steps
    def _upload_resets(self):
        if self._pending is None or not self._pending.any():
            self._pending = None
            return
        m = np.concatenate([self._pending, self._pending]).astype(np.int32)
        self._flags.copy_(self._pinned(torch.from_numpy(m)), non_blocking=True)
        self._flags_set = True
        self._pending = None

    def _host_lengths(self, lengths, Tc):
        """step()'s `lengths` checked -> numpy int32 [B]."""
        B = self.num_streams
        a = lengths.detach().cpu().numpy() if torch.is_tensor(lengths) else np.asarray(lengths)
        if a.dtype.kind not in 'iu':
            raise ValueError('step: lengths must be integers, not %s' % a.dtype)
        if a.shape != (B,):
            raise ValueError('step: lengths needs num_streams (%d) entries' % B)
        if a.min() < 0 or a.max() > Tc:
            raise ValueError('step: lengths must lie in 0..%d (the chunk\'s frames)' % Tc)
        return a.astype(np.int32)

    def _upload_lengths(self, n):
        self._lengths.copy_(self._pinned(torch.from_numpy(np.concatenate([n, n]))), non_blocking=True)

    def _eye_mask(self, eye_mask, Tc):
        """step()'s `eye_mask` checked -> (uint8 [B, Tc, 2] tensor, on the device or on the host (then pinned where the model is on
        the GPU)).  A device tensor is taken as it is: its shape and dtype are host knowledge, its values are never read here."""
        shape = (self.num_streams, Tc, 2)
        if torch.is_tensor(eye_mask) and eye_mask.device.type != 'cpu':
            if eye_mask.device != self.device or eye_mask.dtype not in (torch.bool, torch.uint8):
                raise ValueError('step: a device eye_mask must be a bool or uint8 tensor on %s' % (self.device,))
            if tuple(eye_mask.shape) != shape:
                raise ValueError('step: eye_mask must be [num_streams, Tc, 2] = %s, got %s' % (shape, tuple(eye_mask.shape)))
            eye_mask = eye_mask.contiguous()
            return eye_mask.view(torch.uint8) if eye_mask.dtype == torch.bool else eye_mask
        a = eye_mask.detach().numpy() if torch.is_tensor(eye_mask) else np.asarray(eye_mask)
        if a.dtype.kind not in 'biu':
            raise ValueError('step: eye_mask must be bool or integers, not %s' % a.dtype)
        if a.shape != shape:
            raise ValueError('step: eye_mask must be [num_streams, Tc, 2] = %s, got %s' % (shape, a.shape))
        return self._pinned(torch.from_numpy((a != 0).astype(np.uint8)))

    def _check_calibration(self, chunk, B, Tc):
        """step()'s calibration keys, and what an applying step needs, checked before anything is launched or captured."""
        self._check_collecting(chunk, B, Tc, 'calibration', self._calib_apply, self._store,
                               [('inv_camera_transformation', 'the camera geometry (inv_camera_transformation)')],
                               ('head_R', 'head_R in the chunk: the offset is applied in the head\'s frame'))

    def _check_collecting(self, chunk, B, Tc, name, applied, allocate, geometry, derived):
        """What both calibrations check of a step: <name>_target / <name>_valid, and what a collecting or an applying step needs in
        the chunk -- geometry: (key, its description) pairs; derived: (key, description) of the one a pose form stands in for."""
        target, valid = chunk.get(name + '_target'), chunk.get(name + '_valid')
        if target is None and valid is None and not applied:
            return
        if target is None and valid is not None:
            raise ValueError('step: %s_valid comes with %s_target' % (name, name))
        what = name + '_target' if target is not None else 'an applied ' + name.replace('_', ' ')
        for key, described in geometry:
            if key not in chunk:
                raise ValueError('step: %s needs %s in the chunk' % (what, described))
        if derived[0] not in chunk and not has_pose_form(chunk):
            raise ValueError('step: %s needs %s' % (what, derived[1]))
        if target is not None:
            self._check_chunk_tensor(name + '_target', target, (torch.float32,), (B, Tc, 2))
            allocate()                           # the sample store: allocated here, before any capture
        if valid is not None:
            self._check_chunk_tensor(name + '_valid', valid, (torch.bool, torch.uint8), (B, Tc))

    def _check_chunk_tensor(self, name, t, dtypes, shape, got=True, form=None):
        """One entry of the chunk that a stage reads: a tensor of one of dtypes and of that shape (None: any extent) on the model's
        device, or ValueError('step: <name> must be ...').  form: the entry in words, for one with free extents -- its device is
        then left to the launch's wrapper."""
        if (torch.is_tensor(t) and t.dtype in dtypes and t.dim() == len(shape) and all(n is None or n == m for n, m in zip(shape, t.shape)) and
                (form is not None or t.device == self.device)):
            return
        if form is None:
            form = 'a %s [%s] tensor on %s' % (' or '.join(str(dtype)[len('torch.'):] for dtype in dtypes), ', '.join('%d' % n for n in shape),
                                               self.device)
        raise ValueError('step: %s must be %s%s' % (name, form, ', got %s %s' % (getattr(t, 'dtype', type(t)), tuple(getattr(t, 'shape', ())))
                                                    if got else ''))

    def _set_pose_gate(self, skip_invalid_pose):
        if self._pose_gate_host != (not skip_invalid_pose):
            self._pose_gate_host = not skip_invalid_pose
            self._pose_gate.fill_(self._pose_gate_host)              # a device value: the captured graphs read it, the host never waits

    def _run(self, chunk, return_heatmaps, ragged=False, eye_mask=None, masked=False, render=None, events=None, gate=None, history=None,
             aoi=None, pupil=None, luminance=None, saccades=None, pursuits=None):
        """The one call of EVE._predict_sequence, eager or under capture.  render, events, gate, history, aoi, pupil, luminance: None or the plan of
        that stage's check.  A stage's keyword goes along only when the stage runs, and lengths, the mask's keywords and face_state only
        on a ragged, a masked and a face-landmark step: a step without them makes the call it always made."""
        faced = face_landmarks_key(chunk) is not None
        kw = {'reset': self._flags, 'return_heatmaps': return_heatmaps}
        if ragged or masked or faced:
            kw['lengths'] = self._lengths if ragged else None
        if masked or faced:
            kw.update(masked=masked, eye_mask=eye_mask, pose_gate=self._pose_gate if masked and has_pose_form(chunk) else None)
        if faced:                                # the face-landmark form: the carried head pose goes along
            kw['face_state'] = self._face_pose
        if render is not None:
            kw['render'] = self._render_hook(render, ragged, masked)
        if history is not None:
            kw['history'] = history
        if aoi is not None:
            kw['aoi'] = dict(aoi, **self._aoi_entry(aoi['spec'])['buffers']._asdict())
        if pupil is not None:
            kw['pupil'] = dict(pupil, **self._pupil_entry(pupil['spec'])['buffers']._asdict())
        if luminance is not None:
            kw['luminance'] = luminance
        if self._calib_apply or 'calibration_target' in chunk:       # (neither: the call an uncalibrated EVEStream always made)
            kw['calibration'] = {'kappa': self._calib_kappa, 'ok': self._calib_ok, 'apply': self._calib_apply,
                                 'store': self._store() if 'calibration_target' in chunk else None}
        if self._screen_apply or 'screen_calibration_target' in chunk:      # (neither: no keyword, no launch)
            kw['screen_calibration'] = {'coef': self._screen_coef, 'kind': self._screen_kind, 'apply': self._screen_apply,
                                        'store': self._screen_samples() if 'screen_calibration_target' in chunk else None}
        if events is not None:
            kw['events'] = dict(events, **self._event_buffers()._asdict())
        if saccades is not None:
            kw['saccades'] = dict(saccades, **self._saccade_buffers()._asdict())
        if pursuits is not None:
            kw['pursuits'] = dict(pursuits, **self._pursuit_buffers()._asdict())
        if gate is not None:
            kw['gate'] = dict(gate, **self._gate_buffers()._asdict())
        return self.model._predict_sequence(chunk, self._eye, self._ref, **kw)

    # ------------------------------------------------------------------ the overlay (step(chunk, render=spec))
    def _render_plan(self, chunk, spec, events=None, history=None):
        """step()'s `render` checked against the chunk -> what the launch needs beside the step's own results: the capture's key,
        format and size, the matrix, sx and sy, the marker table on the device, the inset's place.  Every refusal is a ValueError
        raised before anything is launched or captured."""
        from .data import OverlaySpec, eye_patch_hw
        from .kernels import pixel_format_shape
        from .refine_net import SCREEN_FRAME_KEYS, SCREEN_SURFACE_KEY, screen_frame_key
        if not isinstance(spec, OverlaySpec):
            raise ValueError('step: render must be an eve_amd.OverlaySpec, got %s' % type(spec).__name__)
        cfg = self.model.config
        key = screen_frame_key(chunk)
        if key is None:
            raise ValueError('step: render draws onto the screen capture, and the chunk holds none (screen_frame, or one of %s)' %
                             ', '.join(k_ for k_ in SCREEN_FRAME_KEYS if k_ != 'screen_frame'))
        if key == SCREEN_SURFACE_KEY:
            raise ValueError('step: render does not draw onto a %s capture: the overlay reads byte-linear frames (hand the capture over '
                             'under one of %s to render)' % (key, ', '.join(SCREEN_FRAME_KEYS)))
        frames = chunk[key]
        net_hw = (int(cfg.screen_size[1]), int(cfg.screen_size[0]))
        if key == 'screen_frame' and (not torch.is_tensor(frames) or frames.dtype != torch.uint8 or frames.dim() != 5 or
                                      frames.shape[4] not in (3, 4) or tuple(frames.shape[2:4]) == net_hw):
            raise ValueError('step: render needs a full-resolution uint8 capture [B, Tc, IH, IW, 3 | 4] to draw onto; screen_frame is %s %s '
                             '(a float or %d x %d screen_frame is the network\'s input, not a capture)' % (
                                 getattr(frames, 'dtype', type(frames)), tuple(getattr(frames, 'shape', ())), net_hw[0], net_hw[1]))
        fmt = SCREEN_FRAME_KEYS[key]
        try:
            IH, IW, _ = pixel_format_shape(frames, fmt, lead=2, name=key)
        except TypeError as e:
            raise ValueError('step: render: %s' % e)
        if spec.out_format in ('nv12', 'i420') and (IH % 2 or IW % 2):
            raise ValueError('step: render: out_format %s needs a capture of even size, got %d x %d' % (spec.out_format, IH, IW))
        ref = self.model.refine_net
        wants_final = spec.heat or any(m[0] == 'PoG_px_final' for m in spec.markers)
        if wants_final and ref is None:
            raise ValueError('step: render uses %s, which RefineNet produces, and the model has no RefineNet' % (
                'the heat map (heatmap_final)' if spec.heat else 'PoG_px_final'))
        results = tuple(getattr(self.model, 'PREDICTION_KEYS', ())) + ('valid', 'eye_valid', 'pose_valid')
        if events is not None:                   # the gaze events' keys: dict(key='fixation_px', valid='fixating'), key='PoG_px_filtered'
            from .data import GAZE_EVENT_KEYS
            results += GAZE_EVENT_KEYS
        if self._screen_apply:                   # an applied screen map: the uncorrected point can be drawn beside the corrected one
            results += ('PoG_px_%s_raw' % self._output_stage(), 'screen_calibrated')
        if spec.heat_key is not None:            # a gaze history map of this step in place of heatmap_final
            named = [h for h in (history or ()) if h['spec'].name == spec.heat_key]
            if not named:
                raise ValueError('step: render: heat_key %r names no history spec of this step (history=...)' % (spec.heat_key,))
            if not named[0]['spec'].per_frame:
                raise ValueError('step: render: heat_key %r needs a per_frame=True history spec: the overlay blends a map per frame' % (spec.heat_key,))
            if max(named[0]['P']['size']) > 1024:
                raise ValueError('step: render: heat_key %r: the overlay blends maps of up to 1024 per axis, this one is %d x %d' % (
                    (spec.heat_key,) + tuple(named[0]['P']['size'])))
        for m in spec.markers:
            for k_ in (m[0], m[1]):
                if k_ is not None and k_ not in chunk and k_ not in results:
                    raise ValueError('step: render: marker key %r is neither in the chunk nor a result of the step' % (k_,))
        B, Tc = frames.shape[:2]
        inset_hw = None
        if spec.inset == 'eyes':
            if 'left_eye_patch' in chunk:
                p = chunk['left_eye_patch']
                ph, pw = (int(p.shape[2]), int(p.shape[3])) if p.dtype == torch.uint8 else (int(p.shape[3]), int(p.shape[4]))
            else:
                ph, pw = eye_patch_hw(cfg)
            inset_hw = (ph, 2 * pw)
        elif spec.inset is not None:
            p = chunk.get(spec.inset)
            self._check_chunk_tensor('render: inset %r' % (spec.inset,), p, (torch.uint8,), (B, Tc, None, None, 3),
                                     form='a uint8 [B, Tc, h, w, 3] entry of the chunk')
            inset_hw = (int(p.shape[2]), int(p.shape[3]))
        inset_xy = None
        if inset_hw is not None:
            z = spec.inset_zoom
            inset_xy = spec.inset_xy if spec.inset_xy is not None else (IW - z * inset_hw[1], IH - z * inset_hw[0])
            if inset_xy[0] < 0 or inset_xy[1] < 0 or inset_xy[0] + z * inset_hw[1] > IW or inset_xy[1] + z * inset_hw[0] > IH:
                raise ValueError('step: render: the inset (%d x %d at zoom %d, top-left %s) does not lie inside the %d x %d capture' % (
                    inset_hw[0], inset_hw[1], z, tuple(inset_xy), IH, IW))
        table = None
        if spec.markers:
            table = self._render_tables.get(spec.key())
            if table is None:                    # made here, before any capture: a host-to-device copy
                table = self._render_tables[spec.key()] = torch.tensor(spec.marker_table(), dtype=torch.int32).reshape(-1, 4).to(self.device)
        matrix = spec.matrix if spec.matrix is not None else (ref.yuv_matrix if ref is not None else 'bt601')
        return {'spec': spec, 'key': key, 'format': fmt, 'matrix': matrix, 'table': table, 'inset_xy': inset_xy,
                'sx': IW / float(cfg.actual_screen_size[0]), 'sy': IH / float(cfg.actual_screen_size[1])}

    def _render_hook(self, plan, ragged, masked):
        """The closure EVE._predict_sequence calls last: gathers the layers from the step's own tensors and issues the one
        eve_overlay_render launch on the capture where it lies (the chunk tensor; under a graph, its input buffer)."""
        from .data import quantise_patches
        spec = plan['spec']

        def render(d, inter, out):
            frames = d[plan['key']]
            B, Tc = frames.shape[:2]
            N = B * Tc
            flat = frames.reshape((N,) + tuple(frames.shape[2:]))

            def look(key):
                for src in (out, inter, d):
                    if key in src:
                        return src[key]
                raise ValueError('step: render: %r is neither in the chunk nor a result of this step' % (key,))

            kw = {}
            if spec.markers:
                kw['centres'] = torch.stack([look(m[0]).reshape(N, 2).float() for m in spec.markers], dim=1).contiguous()
                kw['marker_table'], kw['sx'], kw['sy'] = plan['table'], plan['sx'], plan['sy']
                if any(m[1] is not None for m in spec.markers):
                    ones = torch.ones((N,), dtype=torch.bool, device=frames.device)
                    kw['marker_valid'] = torch.stack([ones if m[1] is None else look(m[1]).reshape(N) != 0 for m in spec.markers],
                                                     dim=1).to(torch.uint8).contiguous()
            if spec.heat:
                hm = look('heatmap_final')
                kw.update(heat=hm.reshape((N,) + tuple(hm.shape[-2:])).float().contiguous(), heat_color=spec.heat_color, amax=spec.heat_amax)
            elif spec.heat_key is not None:
                hm = out[spec.heat_key + '_frames']
                kw.update(heat=hm.reshape((N,) + tuple(hm.shape[-2:])), heat_color=spec.heat_color, amax=spec.heat_amax)
            if spec.inset == 'eyes':
                if 'left_eye_patch' in d:
                    left, right = d['left_eye_patch'], d['right_eye_patch']
                    left, right = (left[..., :3], right[..., :3]) if left.dtype == torch.uint8 else (quantise_patches(left), quantise_patches(right))
                    h, w = left.shape[2:4]
                    inset = torch.cat([right, left], dim=3).reshape(N, h, 2 * w, 3)
                else:                            # a camera form: the patches once more, in the float form (two launches)
                    _, _, _, _, lw, rw, _, to_nchw = self.model.eye_net._camera_cutters(d)
                    inset = torch.cat([quantise_patches(to_nchw(rw)), quantise_patches(to_nchw(lw))], dim=2)
                kw['inset'] = inset.contiguous()
            elif spec.inset is not None:
                p = d[spec.inset]
                kw['inset'] = p.reshape((N,) + tuple(p.shape[2:]))
            if 'inset' in kw:
                kw.update(inset_xy=plan['inset_xy'], zoom=spec.inset_zoom, mirror=spec.inset_mirror)
            if masked:
                kw['frame_valid'] = out['valid'].reshape(N).to(torch.uint8).contiguous()
            elif ragged:
                kw['frame_valid'] = (torch.arange(Tc, device=frames.device)[None, :] < self._lengths[:B, None]).reshape(N).to(torch.uint8).contiguous()
            rendered = default_kernels().overlay_render(flat, plan['format'], spec.out_format, plan['matrix'], **kw)
            out['rendered'] = rendered.view((B, Tc) + tuple(rendered.shape[1:]))
        return render

    def step(self, chunk, return_heatmaps=False, lengths=None, eye_mask=None, skip_invalid_pose=False, render=None, events=None, gate=None,
             history=None, aoi=None, pupil=None, luminance=None, saccades=None, pursuits=None):
        """One chunk of every stream: chunk holds [B, Tc, ...] tensors on the model's device -- the eyes (below), {left,right}_h,
        {left,right}_o, {left,right}_R, head_R, camera_transformation, inv_camera_transformation, pixels_per_millimeter, millimeters_per_pixel, and screen_frame when the config loads screen content.  Returns the
        prediction keys of EVE(output_predictions=True) as [B, Tc, ...] tensors (heatmap_final [B, Tc, 1, H, W] on request).
        With use_graph the returned tensors are the graph's output buffers: valid until the next step() of the same chunk
        shape (clone what you keep).  The host does not wait for the device, except when a new chunk shape is captured.

        The eyes come as left_eye_patch / right_eye_patch (float NCHW [B, Tc, 3, H, W] or uint8 NHWC [B, Tc, H, W, C], cut
        beforehand), or as what a live camera and a face tracker deliver: camera_frame, uint8 [B, Tc, IH, IW, 3 | 4] whole frames
        up to 16384 x 16384 (a fourth channel ignored, the channel order kept), plus left_eye_warp and right_eye_warp, float32
        [B, Tc, 3, 3]: per frame and eye the homography from a patch pixel to a camera pixel -- cv2.warpPerspective's
        WARP_INVERSE_MAP matrix, inv(W) of the perspective-normalisation matrix W.  The patches (the config's eyes_size) are then
        cut by eve_eye_warp_u8_to_stem / _to_nchw inside the step and inside the captured graph: the frames and the matrices are
        copied into the graph's input buffers like every other tensor of the chunk, and their shapes and dtypes are part of the
        graph's key.  A chunk holds one form, not both.  The camera form may add camera_lens, float32 [B, Tc, 12] rows
        (fx, fy, cx, cy, k1, k2, p1, p2, k3, k4, k5, k6) from data.camera_lens -- the intrinsics and OpenCV distortion coefficients
        of the camera behind each frame, one row for both eyes: camera_frame is then the RAW frame, the warps keep referring to
        the undistorted image the networks were trained on, and eve_eye_warp_lens_u8_to_stem / _to_nchw push every coordinate
        through the lens model before the frame is read (no undistorted frame is made; zero coefficients give the plain bits).
        A chunk with the key captures a graph of its own, and a replay reads the rows of the chunk at hand.

        Or as the pose form, straight from the face tracker: camera_frame plus eye_pose, float32 [B, Tc, 18] rows from data.eye_pose
        = (fx, fy, cx, cy, rvec, tvec, left and right eye centre in the head model, focal_norm, distance_norm) -- cv2.solvePnP's
        result, the camera matrix of the undistorted image and the virtual camera of the patch.  eye_pose then stands in for
        left_eye_warp / right_eye_warp AND for {left,right}_h, {left,right}_o, {left,right}_R and head_R (a chunk that holds one of
        them, or patches, beside eye_pose is refused): one eve_eye_pose_normalize launch derives them for the config's eyes_size by
        the published normalisation procedure the reference cites (data.normalize_eyes has the conventions, the sign of h
        included; none of it could be compared with the EVE dataset's own values).  The launch sits inside the step and inside
        the captured graph, the rows are a graph input like every other chunk tensor -- a replay reads the rows of the chunk at
        hand -- and the key of the graph covers them; ragged steps and camera_lens combine with it unchanged.  The result gains
        pose_valid, bool [B, Tc, 2] (left, right): False where a pose was not usable (a NaN, a head behind the camera, ...), whose
        eye then got a black patch, R = I, o = 0 and h = 0.  pose_valid is reported, not folded into any other validity -- unless
        skip_invalid_pose (below) asks for it.

        Or as the face-landmark form, which needs no solvePnP on the host: camera_frame plus face_landmarks, float32 [B, Tc, L, 2 | 3]
        = pixel (u, v[, w]) of the tracker's L landmarks in the undistorted image (w an optional confidence, 0 drops the point;
        4 <= L <= 68), plus face_rig, float32 [B, 12 + 3L] rows from data.face_rig, ONE PER STREAM (camera matrix, eye centres,
        virtual camera, the L model points).  One eve_face_pose_solve launch inside the step and the graph solves every frame's
        head pose -- a wavefront per stream, each frame started from the one before, the chunk's first frame from the pose this
        EVEStream carries in a float64 [B, 13] buffer (get_head_pose / set_head_pose; reset() clears it through the same device
        flags, inside the same graph) -- and eve_eye_pose_normalize_rt derives what eye_pose derives.  The result gains
        pose_valid as above (False for both eyes of a frame without a solution: a NaN, fewer than 4 weighted points, no
        convergence), head_t [B, Tc, 3] and face_reproj_rms [B, Tc] (pixels).  lengths, eye_mask, skip_invalid_pose, camera_lens and
        the pixel-format keys combine with it; frames past lengths[b] are not solved and leave the carried pose alone.  A split
        of a clip into chunks gives the poses of one pass over the clip, bit for bit.
        A tracker fed the RAW frame of a camera with lens distortion reports raw pixels: pass them as face_landmarks_raw (same
        shape) in place of face_landmarks.  It requires camera_lens, whose rows then undistort both the pixels (inside the warp)
        and the points (inside the solve's launch, by Newton's method: a few 1e-16 in normalised coordinates; a point it cannot
        invert is dropped); both landmark keys together, or the raw key without camera_lens, raise ValueError; face_landmarks +
        camera_lens keeps meaning landmarks of the undistorted image.  model.eye_net.face_huber_px = k (None, or pixels > 0;
        anything else raises ValueError) gives the solve a Huber loss: landmarks further than k from their reprojection are
        down-weighted, so a few that are confidently wrong (a hand, hair across the face) no longer tilt the head -- at L = 68
        with 7 of them moved 30..80 px, 0.35 degrees median where the plain solve has 3.1.  A frame that ends with fewer than 4
        landmarks within k is invalid.  With either, the launch is eve_face_pose_solve_ex and the result gains face_inliers,
        uint8 [B, Tc]: the landmarks within k (the used ones without the loss), 0 where invalid; face_reproj_rms stays the rms
        over all used landmarks.  The value is part of the graph's key: changing the attribute captures a new graph.  Not
        promised: six landmarks with an outlier among them.  Not offered: RANSAC, per-frame rigs, fisheye / thin-prism / tilt
        lens models.

        screen_frame is float [B, Tc, 3, H, W] at the configured screen size, uint8 [B, Tc, H, W, 3] at that size, or a live
        capture as it comes off the desktop: uint8 [B, Tc, IH, IW, 3 | 4] at any resolution from the screen size up to 16 843 009
        pixels (3840 x 2160 included), area-averaged down on the device by eve_screen_u8_area_to_nchw inside the step -- and
        inside the captured graph, whose key holds the capture's shape and dtype.  A fourth channel (BGRA's alpha) is ignored;
        the channel order is kept.  A BGR(A) capture, what capture APIs and OpenCV deliver, goes under screen_frame_bgr instead
        (uint8 [B, Tc, IH, IW, 3 | 4], never beside screen_frame): eve_screen_u8_area_bgr_to_nchw reads channel 2 - c into plane c, and
        the step equals the one on the channel-reversed capture bit for bit.  A decoder's or a capture path's YUV surface goes
        under ONE of these keys in place of screen_frame (uint8, contiguous, byte-linear per frame; two screen keys raise ValueError):
          screen_frame_nv12  [B, Tc, IH*3/2, IW]      luma rows, then IH/2 rows of interleaved U, V (hardware decoders); IH, IW even
          screen_frame_i420  [B, Tc, IH*3/2, IW]      luma, the U plane, the V plane (ffmpeg's yuv420p); IH, IW even
          screen_frame_yuyv  [B, Tc, IH, IW, 2]       Y U Y V per pixel pair; IW even
        eve_screen_area_fmt_to_nchw converts every pixel as the area resize reads it -- chroma the nearest sample, the bit-exact
        integer matrix model.refine_net.yuv_matrix names ('bt601' default; HD recordings are usually 'bt709'; 'jfif') -- and
        averages the converted values, inside the step and the captured graph, whose input buffer holds the surface as it came
        (NV12 / I420: 3.1 MB per 1080p frame where RGB has 6.2 MB, YUYV 4.1 MB) and whose key holds the matrix.  The step equals the
        screen_frame step on the converted RGB capture bit for bit; lengths, eye_mask, every camera form and the camera
        pixel-format keys combine with these keys unchanged.

        In both camera forms the frames may come in the layout the camera or decoder delivers, under ONE of these keys in place of
        camera_frame (uint8, contiguous, byte-linear per frame; two frame keys raise ValueError):
          camera_frame_bgr   [B, Tc, IH, IW, 3 | 4]   channel 2 red, channel 0 blue, a fourth ignored (OpenCV, capture APIs)
          camera_frame_nv12  [B, Tc, IH*3/2, IW]      luma rows, then IH/2 rows of interleaved U, V (hardware decoders); IH, IW even
          camera_frame_i420  [B, Tc, IH*3/2, IW]      luma, the U plane, the V plane (ffmpeg's yuv420p); IH, IW even
          camera_frame_yuyv  [B, Tc, IH, IW, 2]       Y U Y V per pixel pair (UVC webcams' YUY2); IW even
        eve_eye_warp_fmt_to_stem / _to_nchw then convert the four taps of each output pixel as they read them -- chroma the nearest
        sample, the bit-exact integer matrix model.eye_net.yuv_matrix names ('bt601' default, 'bt709', 'jfif') -- inside the step
        and the captured graph, whose input buffer holds the frame as it came (NV12 / I420: half of RGB's bytes, YUYV two thirds)
        and whose key holds the matrix.  The step equals the camera_frame step on the converted frame bit for bit; camera_lens,
        eye_pose, lengths, eye_mask and skip_invalid_pose combine with these keys unchanged.

        A decoder's or a capture API's SURFACE goes in as it lies in memory -- rows with a pitch, more coded rows than visible
        ones, chroma planes at aligned offsets, a window of a larger texture; NV21, YV12, UYVY, P010 (read as its high byte: the
        sample >> 8, a truncation) and pitched RGB(A) / BGR(A) beside the formats above -- under one more key on each side:
          camera_surface     [B, Tc, rows, pitch] or [B, Tc, frame_bytes]   with model.eye_net.camera_layout
          screen_surface     [B, Tc, rows, pitch] or [B, Tc, frame_bytes]   with model.refine_net.screen_layout
        each layout a data.SurfaceLayout(format, width, height, pitch=, coded_height=, x0=, y0=, plane_offsets=); a surface key
        without its layout is a ValueError, two frame keys on one side too.  eve_eye_warp_surface_to_stem / _to_nchw read the
        four taps of an output pixel, and eve_screen_area_surface_to_nchw every visible pixel, through the layout's address rule
        inside the step and the captured graph: the graph's input buffer is the surface copied whole, padding included (no
        de-pitch, crop or byte-shuffle pass runs before the step), and both layouts are part of the graph's key.  The step equals
        the one on the de-pitched, cropped, byte-linear frames under their format's key bit for bit; camera_lens, eye_pose,
        face_landmarks, lengths, eye_mask and skip_invalid_pose combine unchanged.  render= with a screen_surface chunk is
        refused (ValueError): the overlay reads byte-linear captures.  Not offered: planes in separate allocations, bottom-up
        (negative-pitch) images, tiled or compressed surfaces, 10-bit arithmetic, bilinear chroma up-sampling -- for the camera
        and for the screen alike.

        lengths: None, or num_streams integers in 0..Tc (list, numpy array or CPU tensor) for streams that delivered different
        numbers of frames: stream b consumes frames 0..lengths[b]-1 of the chunk, and every carried state of it afterwards is the
        state after exactly that many frames -- untouched for 0 frames, except that a requested reset() is still applied.  The
        outputs keep their [B, Tc, ...] shapes, their entries at t >= lengths[b] are unspecified, and the result gains `valid`, a
        bool [B, Tc] device tensor that marks the consumed frames.  The frames past a stream's count are computed like real ones:
        the step costs what a full chunk of this shape costs.

        eye_mask: None, or [B, Tc, 2] with columns (left, right), True / non-zero = the eye is usable in that frame: a bool or
        uint8 tensor on the model's device (used as it is: a tracker on the GPU causes no host sync), or a CPU tensor, a numpy
        array or nested lists of bools / integers (checked on the host -- a wrong shape or a float dtype raises ValueError -- and
        uploaded like lengths and resets: a pinned block, an asynchronous copy, never baked into a graph).  skip_invalid_pose=True
        (the pose form only: ValueError without eye_pose in the chunk) ANDs pose_valid into the mask on the device.  Eye (b, t,
        side) is usable iff mask[b, t, side] and t < lengths[b] (and pose_valid[b, t, side] with skip_invalid_pose); frame (b, t)
        is valid iff at least one of its eyes is usable.  The contract of a masked step:
          * EyeNet: sequence (b, side) consumes exactly its usable frames, in order; its carried state afterwards is the state
            after those frames -- untouched for none, except that a requested reset() is still applied.  Every tail variant
            (GRU / RNN / LSTM, stacked, wide, STATIC, stream_fused_tail).
          * RefineNet: stream b consumes exactly its valid frames; its cell states are held across the others and committed
            from the last valid one (every cell type, stacked cells, every width, refine_net_clstm_feeds_features).
          * On a valid frame PoG_px_initial / PoG_cm_initial are the two eyes' mean where both are usable (today's bits) and the
            usable eye's own PoG where one is; o is the mean of the usable origins; the rotation behind g_initial and g_final is
            left_R where the left eye is usable, else right_R -- an approximation the reference never needed.  Nothing a
            masked-out eye supplied (patch, h, o, R, warp, pose) reaches a valid output: the choice is made by selects on the
            device, so not even a NaN there does.
          * The outputs keep their [B, Tc, ...] shapes; entries at invalid frames, and per-eye entries (<side>_g_initial,
            <side>_pupil_size) at unusable eyes, are unspecified.  The result gains valid, bool [B, Tc], and eye_valid, bool [B,
            Tc, 2]: the effective mask after lengths and pose_valid.
          * Masked frames are computed like real ones (no compute is skipped): the step costs a full chunk plus one plan launch,
            six small row gathers and ten elementwise selects (profiles/stream_mask_notes.md).  The mask is one more input
            buffer of the graph: one masked graph per chunk shape serves every mask pattern.
        A step with neither argument issues exactly the kernel calls it always did.

        render: None, or an eve_amd.OverlaySpec -- the result gains `rendered`, the chunk's full-resolution screen capture
        (whichever screen_frame* key holds it; a float or network-sized screen_frame is refused: a capture is needed) annotated
        on the device by one eve_overlay_render launch at the end of the step and inside the captured graph: uint8 [B, Tc, IH, IW, 3]
        for out_format 'rgb' / 'bgr', [B, Tc, IH*3/2, IW] for 'nv12' / 'i420', a graph output buffer like the others.  The launch
        reads the capture where it lies (the graph's input buffer: nothing is copied).  Markers are read from the step's own result
        (PoG_px_initial, PoG_px_final) or the chunk (a caller's PoG_px_gt), in actual_screen_size pixels, and scaled by the capture's
        size over actual_screen_size; heat=True blends this step's heatmap_final (returned or not); inset='eyes' shows the eye
        patches as [right | left]: uint8 patch chunks as they are, float patches quantised by clamp(rint((p + 1) * 127.5), 0, 255),
        and in the camera forms the patches cut once more in the float form (two more eye-warp launches) and quantised the same
        way.  On a ragged or masked step `valid` is the launch's frame_valid: a frame that was not consumed comes out as the bare
        converted capture.  PoG_px_final and the heat map need RefineNet (ValueError without).  The spec is part of the graph's
        key; tests/overlay_ref.py states the arithmetic, exact to the bit.  Not offered: the reference's residual lines from an
        estimate to the ground truth, its legend text, gaze-ray arrows on the eye image, row pitches, 10-bit surfaces, a gradient.
        render=None issues exactly the launches the step always issued.

        calibration_target, float32 [B, Tc, 2] on the model's device -- the dot the person was asked to look at, in
        actual_screen_size pixels -- and optionally calibration_valid, bool or uint8 [B, Tc] (default: every frame), make this a
        collecting step: one eve_calib_append launch inside the step and the graph appends every usable (frame, eye) to this
        EVEStream's sample store -- usable iff calibration_valid, t < lengths[b], eye_valid[b, t, side] on a masked step, every
        input finite and the target in front of the eye -- in frame order, from the network's own angles.  The keys' shapes
        and dtypes are part of the graph's key like any chunk tensor's, so a collecting step has a graph of its own; lengths,
        eye_mask, skip_invalid_pose, every camera and screen form and render combine with it.  Needs inv_camera_transformation and
        head_R in the chunk (the pose forms derive head_R): ValueError otherwise, as for calibration_valid without a target.
        Once fit_calibration or set_calibration has been called the step applies the stored offsets (module docstring,
        "Calibration"): the result gains calibrated [B] and <side>_g_initial_raw, and needs head_R too.

        screen_calibration_target, float32 [B, Tc, 2] on the model's device -- the dot the person was asked to look at, in
        actual_screen_size pixels -- and optionally screen_calibration_valid, bool or uint8 [B, Tc] (default: every frame), make this
        a collecting step of the screen-space map (module docstring, "Screen-space calibration"): one eve_screen_calib_append launch
        after the step's output point PoG_px_<out> is known (<out>: final with a RefineNet, else initial), inside the graph, appends
        every usable frame -- usable iff screen_calibration_valid, t < lengths[b], valid[b, t] on a masked step, every input finite,
        pixels_per_millimeter > 0 and the eye off the screen plane -- in frame order, from the UNCORRECTED point.  The keys are part
        of the graph's key like any chunk tensor's; they are not calibration_target (kappa's collector reads the raw angles; one
        chunk may carry both).  Needs inv_camera_transformation, pixels_per_millimeter and the origins (left_o, right_o, or a pose
        form): ValueError otherwise, as for screen_calibration_valid without its target.  Once fit_screen_calibration or
        set_screen_calibration has been called the step corrects its output point by one eve_screen_calib_apply launch, before the
        events stage and the render hook: PoG_px_<out> is the corrected point, PoG_cm_<out> and g_<out> follow, and the result gains
        PoG_px_<out>_raw and screen_calibrated [B]; it then needs millimeters_per_pixel and camera_transformation too.

        events: None, or an eve_amd.GazeEventSpec -- one eve_gaze_events launch at the end of the step (before the overlay) and inside
        the captured graph post-processes the step's point of gaze (spec.source: PoG_px_final with a RefineNet, else
        PoG_px_initial) the way every consumer of an eye tracker does, with no host sync and with state carried from step to step
        like the recurrent states.  The result gains PoG_px_filtered float32 [B, Tc, 2] (a one-euro filter, x and y on their own),
        gaze_velocity float32 [B, Tc] (degrees / second: the angle at the eye -- the step's binocular origin o -- between the gaze
        vectors of consecutive samples over their time difference; NaN where there is none), gaze_event uint8 [B, Tc] (0 none, 1
        fixation, 2 saccade: velocity above spec.saccade_deg_s), fixation_id int32 [B, Tc] (-1 outside a fixation; a counter per
        stream that reset() leaves running), fixation_px float32 [B, Tc, 2] (the running fixation's centroid of the unfiltered
        source), fixation_ms float32 [B, Tc] and fixating uint8 [B, Tc] (a fixation that has lasted spec.min_fixation_s).  A frame
        is a sample iff it was delivered (lengths), is valid (eye_mask, skip_invalid_pose), its PoG, o, inv_camera_transformation and
        pixels_per_millimeter are finite, the eye is off the screen plane and its time is later than the last sample's; any other
        frame is event 0 and moves nothing.  Time is the chunk's frame_time, float64 [B, Tc] seconds on the model's device, or
        frames / spec.fps counted over the delivered frames since the stream's last reset (frame_time wins).  Two samples more
        than spec.max_gap_s apart are not connected: the open fixation ends at its last sample and the filter restarts (so does the
        first sample after a reset()).  A fixation that ends -- a saccade, a gap, reset(), flush_fixations() -- after at least
        min_fixation_s goes to this EVEStream's store (fixation_capacity rows per stream; a full store drops and counts):
        fixations(), fixation_counts(), clear_fixations(); get_event_state() / set_event_state() hold the carried row.  Needs
        inv_camera_transformation, pixels_per_millimeter, the origins (or a pose form), and frame_time or spec.fps: ValueError
        otherwise, as for PoG_px_final without a RefineNet.  The spec by value and frame_time's presence are part of the graph's
        key; lengths, eye_mask, skip_invalid_pose, every camera and screen form, an applied calibration and render combine with it,
        and render's markers may name the new keys (dict(key='fixation_px', valid='fixating'), key='PoG_px_filtered').
        tests/gaze_events_ref.py states the arithmetic.  What is not offered: module docstring, "Gaze events".  events=None issues
        exactly the launches the step always issued.

        gate: None, or an eve_amd.EyeGateSpec -- one eve_eye_gate launch after the pose derivation and before the mask plan, inside the
        captured graph, decides per frame and eye whether the eye is usable, and that verdict is the step's eye_mask (ANDed with
        an eye_mask of the caller's): the step is a masked step with everything that says (valid, eye_valid, the contract above),
        and pose_valid always counts where a pose form is in the chunk, as with skip_invalid_pose.  The criteria (data.EyeGateSpec;
        all off by default): face_reproj_rms <= max_reproj_px and face_inliers >= min_inliers (the face-landmark form; the latter
        with eye_net.face_huber_px or face_landmarks_raw), at least min_coverage of an 8 x 8 lattice over the patch inside the
        camera frame (any camera form; the size comes from the frame key's shape or eye_net.camera_layout; with camera_lens in
        the undistorted coordinates the warp refers to, an approximation at the edge), <side>_h within head_pitch and the eye's
        own head_yaw_left / head_yaw_right (any camera form), and blink, a data.BlinkSpec: the chunk's eye_contours, float32
        [B, Tc, 2, 6, 2 | 3] on the model's device -- pixel (u, v[, w]) of the six eyelid points p1 .. p6 of the (left, right) eye,
        p1 and p4 the corners, p2 and p3 on the upper lid, p6 and p5 below them -- give the aspect ratio ear = (|p2-p6| + |p3-p5|) /
        (2 |p1-p4|), unknown with a non-finite coordinate, a weight <= 0 or no width.  The first known ear is the baseline, which
        follows the open eye (baseline_rise upwards, baseline_rate downwards); eye_openness = ear / baseline; below close_ratio
        the eye closes, above open_ratio it reopens, the blink (eye, first tick, last tick, minimum openness) goes to the store
        and hold_frames frames from the reopening one on are withheld; a closure longer than max_closed_frames starts the
        baseline over and stores nothing; an unknown ear moves nothing.  A tick counts the stream's delivered frames since its
        last reset(); frames past lengths[b] are not delivered.  The result gains eye_gate_reason uint8 [B, Tc, 2] (1 pose, 2
        reprojection, 4 inliers, 8 coverage, 16 head angle, 32 closed, 64 hold-off; 0 = usable), eye_openness float32 [B, Tc, 2] and
        blink uint8 [B, Tc, 2].  eye_contours works with pre-cut patches too.  A criterion whose input the chunk or the model does
        not provide, a blink without eye_contours, and eye_contours of another dtype, shape or device are ValueErrors raised
        before anything is launched or captured.  The spec by value and eye_contours' shape are part of the graph's key; lengths,
        eye_mask, every camera and screen form, calibration, events and render combine with it.  What is not offered: module
        docstring, "The eye gate".  gate=None issues exactly the launches the step always issued.

        history: None, an eve_amd.GazeHistorySpec, or a list of up to two with distinct names -- per spec one eve_gaze_history_plan and
        one eve_gaze_history_update launch after the screen-space map and the events stage and before the overlay, inside the captured
        graph, accumulate the time-decayed history of the point of gaze (module docstring, "Gaze history"): M_t = decay_per_ms^(ms
        since the previous frame) * M_{t-1} + w_t * G_t per stream.  The result gains <name>, float32 [B, MH, MW] -- the map after the
        stream's last consumed frame of the chunk -- and with per_frame <name>_frames, float32 [B, Tc, MH, MW] (frames past a ragged
        length hold unspecified values).  spec.source: PoG_px_final with a RefineNet, else PoG_px_initial; PoG_px_filtered and
        fixation_px need events= in the same step; heatmap_final needs a RefineNet and size == gaze_heatmap_size.  spec.valid_key names
        a bool / uint8 [B, Tc] entry of the chunk, or `fixating` (with events=) or `valid` (a masked step).  A frame is usable iff it
        was delivered (lengths), is valid (eye_mask, gate=, skip_invalid_pose), its valid_key holds and its point is finite; a frame
        that is not decays the map and deposits nothing.  Time is the chunk's frame_time, float64 [B, Tc] seconds, or frames /
        spec.fps counted over the delivered frames since the stream's last reset (frame_time wins); a frame whose time is not finite
        or lies before the previous one's is ignored.  The map is carried from step to step and cleared by reset(); it is tied to
        its spec (ValueError for a known name under another spec: clear_gaze_history first).  The specs by value, the config's
        defaults resolved, are part of the graph's key; lengths, eye_mask, gate=, events=, both calibrations, every camera and screen
        form and render combine with it, and OverlaySpec(heat_key=<name>) blends the per_frame map of that name in place of
        heatmap_final (a map with an axis above 1024, one without per_frame, and heat_key beside heat=True are ValueErrors).  The host
        does not wait.  tests/gaze_history_ref.py states the arithmetic, exact to the bit.  What is not offered: module docstring,
        "Gaze history".  history=None issues exactly the launches the step always issued.

        aoi: None, or an eve_amd.AoiSpec -- one eve_gaze_aoi launch after the events and history stages and before the overlay, inside the
        captured graph, tests the step's point of gaze against the chunk's aoi_shapes, float32 [B, A, 36] or [B, Tc, A, 36] (one table per
        frame, for regions that move) on the model's device, A = spec.num_aois (data.aoi_shapes builds a table; module docstring, "Areas
        of interest").  The result gains <name>_id int32 [B, Tc] (the lowest row that contains the point; -1 none; -2 the frame is not a
        sample), <name>_mask int64 [B, Tc] (bit a: row a contains the point) and <name>_visit_ms float32 [B, Tc] (the time since the
        running visit began).  spec.source: PoG_px_final with a RefineNet, else PoG_px_initial -- the corrected point where a screen-space
        map is applied; PoG_px_filtered and fixation_px need events= in the same step.  spec.valid_key names a bool / uint8 [B, Tc] entry
        of the chunk, or `fixating` (with events=) or `valid` (a masked step).  A frame is a sample iff it was delivered (lengths), is
        valid (eye_mask, gate=, skip_invalid_pose), its valid_key holds, its point and time are finite and the time is later than the
        last sample's.  Time is the chunk's frame_time, float64 [B, Tc] seconds, or frames / spec.fps counted over the delivered frames
        since the stream's last reset (frame_time wins).  With events= (unless use_fixations=False) fixations are counted per AOI and
        per visit.  The dwell table, the transitions and the visit store are carried on the device: aoi_table(), aoi_transitions(),
        aoi_visits(), aoi_visit_counts(), clear_aoi(), flush_aoi_visits(), get_aoi_state() / set_aoi_state(); reset() closes the open
        visit and keeps the tallies, which are tied to their spec (ValueError for a known name under another spec: clear_aoi first).
        ValueErrors raised before anything is launched or captured: aoi_shapes missing or of another shape, dtype or device, a source
        or valid_key the step does not produce, use_fixations=True without events=, neither frame_time nor fps, a name whose keys
        collide with the chunk's or the result's.  The spec by value and aoi_shapes' shape are part of the graph's key; lengths,
        eye_mask, gate=, events=, history=, both calibrations, every camera and screen form and render combine with it.
        tests/aoi_ref.py states the arithmetic, exact to the bit.  aoi=None issues exactly the launches the step always issued.

        pupil: None, or an eve_amd.PupilSpec -- one eve_pupil_track launch after the AOI stage and before the overlay, inside the
        captured graph, turns the step's own left_pupil_size / right_pupil_size into one validated, fused, low-passed, light- and
        baseline-corrected trace per stream (module docstring, "Pupillometry").  On a masked or gated step the eyes the mask plan
        withheld (eye_mask, gate=, a blink and its hold-off, skip_invalid_pose) are withheld here; their sizes are never read into
        any arithmetic.  Optional chunk keys, graph inputs like aoi_shapes: pupil_luminance float32 [B, Tc] (the light covariate, e.g.
        an ambient sensor's reading or the caller's own screen mean) and pupil_baseline bool / uint8 [B, Tc] (the frames that form the
        baseline; a new run of marks starts a new one).  The result gains <name>_mm, _raw_mm, _velocity (mm/s), _change_mm, _change_pct
        float32 [B, Tc] -- NaN where the frame is no sample, and the two changes NaN while there is no baseline -- <name>_valid and
        <name>_event (0 none, 1 dilating, 2 constricting) uint8 [B, Tc], <name>_eye_used and <name>_eye_reason (1 withheld, 2 not
        finite, 4 range, 8 speed) uint8 [B, Tc, 2].  Time is the chunk's frame_time or frames / spec.fps, as for the AOI stage.  The
        table, the light response and the episode store are carried on the device: pupil_table(), pupil_episodes(),
        pupil_episode_counts(), clear_pupil(), flush_pupil_episodes(), set_ / get_ / clear_ / fit_pupil_light_response(),
        get_pupil_state() / set_pupil_state(); reset() closes the open episode and keeps the table, which is tied to its spec
        (ValueError for a known name under another spec: clear_pupil first).  ValueErrors raised before anything is launched or
        captured: a pupil that is no PupilSpec, a name whose keys collide with the chunk's or the result's, pupil_luminance or
        pupil_baseline of another shape, dtype or device, neither frame_time nor fps.  The spec by value and the presence of the two
        chunk keys are part of the graph's key; every other mode of the step combines with it.  tests/pupil_ref.py states the
        arithmetic, exact to the bit.  pupil=None issues exactly the launches the step always issued.
        luminance: None, or an eve_amd.ScreenLuminanceSpec -- one eve_screen_luminance launch after the AOI stage and before the pupil
        stage, inside the captured graph, reads the screen capture where it lies (the chunk tensor; under a graph, its input buffer):
        every pixel through a tight SurfaceLayout of its key's format (screen_frame with four channels: 'rgba'; screen_surface through
        model.refine_net.screen_layout), converted with refine_net.yuv_matrix ('bt601' without a RefineNet), linearised through the
        spec's response table, weighted and summed in integers, over the whole screen and over discs of spec.radii_px around the
        spec's source point.  The result gains <name> float32 [B, Tc], with radii <name>_gaze [B, Tc, R], and with to_pupil
        <name>_covariate [B, Tc], which a pupil= stage of the same step takes as its luminance.  The whole-screen column follows
        lengths only -- the screen does not care about the eyes --, the discs also the masked step's valid and the spec's valid_key;
        what is not delivered, a disc without a valid centre and a disc off the screen are NaN, which the pupil stage ignores.
        ValueErrors raised before anything is launched or captured: a luminance that is no ScreenLuminanceSpec, no capture in the
        chunk, a float or network-size screen_frame, to_pupil together with pupil_luminance in the chunk, PoG_px_filtered or
        fixation_px as the source without events=, a name whose keys collide with the chunk's or the result's, radii that fall
        together at the capture's scale.  The spec by value is part of the graph's key; the stage carries no state.
        tests/screen_luminance_ref.py states the arithmetic, exact to the bit.  luminance=None issues exactly the launches the step
        always issued.
        saccades: None, or an eve_amd.SaccadeSpec, with events= in the same step (ValueError without, raised before anything is
        launched) -- the events launch becomes eve_gaze_events_ex, which also hands out its sample flags, sample times and gaze
        vectors (they stay internal), and one eve_gaze_saccades launch right after it, before the history stage and inside the
        captured graph, cuts the runs of saccade frames into events (module docstring, "Saccades").  The result gains saccade_id
        int32 [B, Tc] (-1 outside a saccade; a counter per stream that reset() leaves running, handed out at every onset whether the
        saccade is accepted later or not) and saccade_ms float32 [B, Tc] (the time since the onset: the flag saccadic suppression
        needs is saccade_id >= 0).  A saccade opens at the sample before its first saccade frame and lands at its last saccade frame;
        it is judged when the next fixation frame arrives -- interrupted (more than max_missing frames inside it were no sample),
        long, short, small, or accepted -- and an accepted one goes to the table and the store: saccades(), saccade_counts(),
        saccade_table(), clear_saccades(), get_saccade_state() / set_saccade_state(), data.main_sequence().  A gap, a reset() and a
        restart of the chain abort an open saccade (tallied, not stored); there is no flush: an open saccade has no landing.  The
        amplitude is that of the point the velocity is from (GazeEventSpec.velocity_from).  The spec by value is part of the graph's
        key; every other mode of the step combines with it.  After events steps without saccades= the stage's row is brought back in
        step by one launch with no frames before the next saccades step: a saccade under way then is not reported.
        tests/saccade_ref.py states the arithmetic.  saccades=None issues exactly the launches the step always issued,
        eve_gaze_events included.
        pursuits: None, or an eve_amd.PursuitSpec, with events= in the same step (ValueError without, raised before anything is
        launched) -- smooth pursuit as the third gaze class (module docstring, "Smooth pursuit").  The events launch becomes
        eve_gaze_events_ex, as for saccades=, and one eve_gaze_pursuits launch follows it (and the saccade launch, where there is
        one), before the history stage and inside the captured graph.  The result gains gaze_class uint8 [B, Tc] (0 none, 1
        fixation, 2 saccade, 3 pursuit; gaze_event and the fixation keys keep their bits), pursuit_id int32 [B, Tc] (-1 outside an
        episode; a counter per stream that reset() leaves running), pursuit_ms float32 [B, Tc] (the time since the onset),
        gaze_velocity_windowed and gaze_straightness float32 [B, Tc] (the window's degrees / second and its angle over its path; NaN
        without a window) and pursuit_gain float32 [B, Tc] (NaN without a defined gain).  With pursuit_target in the chunk (float32
        [B, Tc, 2]: the pursued object's position in actual_screen_size pixels, NaN where there is none; its presence is part of
        the graph's key) the gain is the eye's displacement over the window projected on the target's, over the target's, and an
        episode's row holds its mean and the mean distance to the target.  An episode ends at its last pursuit frame when a
        fixation frame that is no candidate or a saccade frame arrives, and is judged then -- interrupted, short, small, or accepted
        -- and an accepted one goes to the table and the store: pursuits(), pursuit_counts(), pursuit_table(), clear_pursuits(),
        get_pursuit_state() / set_pursuit_state(), data.pursuit_summary().  A gap, a reset() and a restart of the chain abort an open
        episode; one open at the end of a chunk goes on in the next.  After events steps without pursuits= the stage's row is
        brought back in step by one launch with no frames before the next pursuits step.  tests/pursuit_ref.py states the
        arithmetic.  pursuits=None issues exactly the launches the step always issued."""
        if self.model.training:
            raise ValueError('EVEStream runs inference only: the model was switched to training mode')
        B, Tc = eye_input(chunk).shape[:2]
        if B != self.num_streams:
            raise ValueError('chunk has %d streams, the EVEStream %d' % (B, self.num_streams))
        ragged = lengths is not None
        masked = eye_mask is not None or bool(skip_invalid_pose) or gate is not None
        if skip_invalid_pose and not has_pose_form(chunk):
            raise ValueError('step: skip_invalid_pose needs the pose form (eye_pose in the chunk): there is no pose_valid to fold in')
        if ragged:
            lengths = self._host_lengths(lengths, Tc)
        if eye_mask is not None:
            eye_mask = self._eye_mask(eye_mask, Tc)
        if events is not None:
            events = self._check_events(chunk, events, B, Tc)
        if gate is not None:
            gate = self._check_gate(chunk, gate, B, Tc)
        more = {} if gate is None else {'gate': gate}      # the keyword goes along only then: a step without it calls what it always did
        if saccades is not None:
            more['saccades'] = saccades = self._check_saccades(saccades, events)
        if pursuits is not None:
            more['pursuits'] = pursuits = self._check_pursuits(chunk, pursuits, events, B, Tc)
        if history is not None:
            more['history'] = history = self._check_history(chunk, history, events, masked, B, Tc)
        if aoi is not None:
            more['aoi'] = aoi = self._check_aoi(chunk, aoi, events, history, masked, B, Tc)
        if pupil is not None:
            more['pupil'] = pupil = self._check_pupil(chunk, pupil, events, history, aoi, gate, B, Tc)
        if luminance is not None:
            more['luminance'] = self._check_luminance(chunk, luminance, events, history, aoi, pupil, gate, masked, B, Tc)
        if render is not None:
            render = self._render_plan(chunk, render, events, history)
        self._check_calibration(chunk, B, Tc)
        self._check_screen_calibration(chunk, B, Tc)
        if history is not None:
            self._history_buffers(history)
        if aoi is not None:
            self._aoi_entry(aoi['spec'])         # the carried buffers, made here: after every refusal, before any capture
        if pupil is not None:
            self._pupil_entry(pupil['spec'])     # likewise
        if ragged:
            self._upload_lengths(lengths)
        if masked and has_pose_form(chunk):
            self._set_pose_gate(bool(skip_invalid_pose))
        self._upload_resets()
        if events is not None:
            self._events_spec = events['spec']
        if saccades is not None:
            self._saccades_spec = saccades['spec']
            if self._saccades_stale:             # the events chain moved on without the stage: every row starts afresh, eagerly
                self._reset_saccade_rows(torch.ones((B,), dtype=torch.int32, device=self.device))
                self._saccades_stale = False
        elif events is not None and self._saccades is not None:
            self._saccades_stale = True
        if pursuits is not None:
            self._pursuits_spec = pursuits['spec']
            if self._pursuits_stale:             # likewise: every pursuit row starts afresh, eagerly
                self._reset_pursuit_rows(torch.ones((B,), dtype=torch.int32, device=self.device))
                self._pursuits_stale = False
        elif events is not None and self._pursuits is not None:
            self._pursuits_stale = True
        if self._flags_set:
            self._reset_idle_stages(events, gate, history, aoi, pupil, saccades, pursuits)
        with torch.no_grad():
            if self.use_graph:
                entry = self._graph_for(chunk, bool(return_heatmaps), ragged, masked, render, events, **more)
                for key, buf in entry['inputs'].items():
                    buf.copy_(chunk[key], non_blocking=True)
                if masked:
                    if eye_mask is None:
                        entry['eye_mask'].fill_(1)
                    else:
                        entry['eye_mask'].copy_(eye_mask, non_blocking=True)
                entry['graph'].replay()
                out = dict(entry['outputs'])
            else:
                if eye_mask is not None and eye_mask.device != self.device:
                    eye_mask = torch.empty(eye_mask.shape, dtype=torch.uint8, device=self.device).copy_(eye_mask, non_blocking=True)
                out = self._run(chunk, return_heatmaps, ragged, eye_mask, masked, render, events, **more)
            if ragged and not masked:
                out['valid'] = torch.arange(Tc, device=self.device)[None, :] < self._lengths[:self.num_streams, None]
        if self._flags_set:
            self._flags.zero_()
            self._flags_set = False
        return out

    # ------------------------------------------------------------------ graphs
    def invalidate(self):
        """Drop every captured graph (and the modules' packs): for weights changed without torch seeing it."""
        self._graphs = {}
        self.model.eye_net.invalidate_packs()
        if self.model.refine_net is not None:
            self.model.refine_net.invalidate_packs()

    def _weights_key(self):
        return tuple(_module_key(m) for m in (self.model.eye_net, self.model.refine_net) if m is not None)

    def _graph_key(self, chunk, return_heatmaps, ragged=False, masked=False, render=None, events=None, gate=None, history=None, aoi=None,
                   pupil=None, luminance=None, saccades=None, pursuits=None):
        """What a captured graph is good for: the step's mode, both YUV matrices, both surface layouts (by value), the overlay
        (render: None or a _render_plan -- its OverlaySpec by value), with a face-landmark form eye_net.face_huber_px (a launch
        argument, so baked in), the gaze events (events: None or a _check_events plan -- its GazeEventSpec by value and its source;
        frame_time's presence is a chunk key), the eye gate (gate: None or a _check_gate plan -- its EyeGateSpec by value and the frame size;
        eye_contours' presence and shape are a chunk key), the gaze history (history: None or _check_history's plans -- each GazeHistorySpec by
        value, its source and the launches' scalars, the config's defaults resolved), the areas of interest (aoi: None or a _check_aoi plan -- its
        AoiSpec by value, its source and whether fixations are counted; aoi_shapes' shape is a chunk key), the pupillometry (pupil: None or a
        _check_pupil plan -- its PupilSpec by value; pupil_luminance's and pupil_baseline's presence are chunk keys), the screen luminance
        (luminance: None or a _check_luminance plan -- its ScreenLuminanceSpec by value and its source; the capture's shape is a chunk key and its
        layout and matrix are RefineNet's), the saccades (saccades: None or a _check_saccades plan -- its SaccadeSpec by value), the smooth pursuit (pursuits: None or a _check_pursuits plan -- its PursuitSpec by value and whether the chunk has pursuit_target), whether a calibration is applied (`calibrated`; a collecting step differs by its chunk keys), whether a screen-space map is applied (likewise), and every chunk tensor's key, shape and dtype -- which of the two landmark keys among them."""
        ref = self.model.refine_net
        spec = None if render is None else render['spec'].key()
        layouts = (self.model.eye_net.camera_layout, None if ref is None else ref.screen_layout)
        huber = None
        if face_landmarks_key(chunk) is not None:      # (checked here too: a value that is refused never becomes a key)
            from .data import check_huber_px
            huber = check_huber_px(self.model.eye_net.face_huber_px, 'face_huber_px')
        return (return_heatmaps, ragged, masked, self.model.eye_net.yuv_matrix, None if ref is None else ref.yuv_matrix, spec, layouts, huber,
                self._calib_apply, self._screen_apply) + (() if events is None else ((events['spec'].key(), events['source']),)) + \
            (() if gate is None else (('gate', gate['spec'].key(), gate['frame_size']),)) + \
            (() if history is None else (('history',) + tuple((h['spec'].key(), h['source'], tuple(sorted(h['P'].items(), key=lambda kv: kv[0])))
                                                                for h in history),)) + \
            (() if aoi is None else (('aoi', aoi['spec'].key(), aoi['source'], aoi['use_fixations']),)) + \
            (() if pupil is None else (('pupil', pupil['spec'].key()),)) + \
            (() if luminance is None else (('luminance', luminance['spec'].key(), luminance['source']),)) + \
            (() if saccades is None else (('saccades', saccades['spec'].key()),)) + \
            (() if pursuits is None else (('pursuits', pursuits['spec'].key(), pursuits['target']),)) + tuple(sorted((k_, tuple(v.shape), v.dtype) for k_, v in chunk.items() if torch.is_tensor(v)))

    def _graph_for(self, chunk, return_heatmaps, ragged=False, masked=False, render=None, events=None, gate=None, history=None, aoi=None,
                   pupil=None, luminance=None, saccades=None, pursuits=None):
        wk = self._weights_key()
        if wk != self._graphs_key:               # new weights: new packs, new graphs (a replay never reads stale packs)
            self._graphs = {}
            self._graphs_key = wk
        more = {} if gate is None else {'gate': gate}
        if history is not None:
            more['history'] = history
        if aoi is not None:
            more['aoi'] = aoi
        if pupil is not None:
            more['pupil'] = pupil
        if luminance is not None:
            more['luminance'] = luminance
        if saccades is not None:
            more['saccades'] = saccades
        if pursuits is not None:
            more['pursuits'] = pursuits
        key = self._graph_key(chunk, return_heatmaps, ragged, masked, render, events, **more)
        entry = self._graphs.get(key)
        if entry is None:
            entry = self._graphs[key] = self._capture(chunk, return_heatmaps, ragged, masked, render, **more) if events is None else \
                self._capture(chunk, return_heatmaps, ragged, masked, render, events, **more)
            self._graphs_key = self._weights_key()
        return entry

    def _capture(self, chunk, return_heatmaps, ragged=False, masked=False, render=None, events=None, gate=None, history=None, aoi=None,
                 pupil=None, luminance=None, saccades=None, pursuits=None):
        """Capture one step for this chunk shape (train.Trainer._capture's recipe): inputs copied into fixed buffers, two eager
        warm-up steps off the default stream (packs, lazily built filters, allocator) with the carried states put back
        afterwards, the kernels' scratch allocated before the capture, one stream, no side branches.  A masked graph has one more
        input buffer, eye_mask uint8 [B, Tc, 2] (all ones while it is captured; step() fills it before every replay)."""
        static = {k_: v.clone() for k_, v in chunk.items() if torch.is_tensor(v)}
        B, Tc = eye_input(chunk).shape[:2]
        eye_mask = torch.ones((B, Tc, 2), dtype=torch.uint8, device=self.device) if masked else None
        dev_index = self.device.index if self.device.index is not None else torch.cuda.current_device()
        side = _WARMUP_STREAMS.get(dev_index)
        if side is None:
            side = _WARMUP_STREAMS[dev_index] = torch.cuda.Stream(device=dev_index)
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            carried = self._carried()
            snap = [t.clone() for t in carried]
            for _ in range(2):
                self._run(static, return_heatmaps, ragged, eye_mask, masked, render, events, gate, history, aoi, pupil, luminance, saccades, pursuits)
            for t, s_ in zip(carried, snap):
                t.copy_(s_)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        k = default_kernels()
        if hasattr(k, 'prepare_graph_workspace'):
            k.prepare_graph_workspace(self.device)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = self._run(static, return_heatmaps, ragged, eye_mask, masked, render, events, gate, history, aoi, pupil, luminance, saccades, pursuits)
        m = self.model
        keep = (m.eye_net._packs, getattr(m.eye_net, '_stream_w', None), m.refine_net._packs if m.refine_net is not None else None)
        return {'graph': graph, 'inputs': static, 'outputs': out, 'keep': keep, 'eye_mask': eye_mask}
