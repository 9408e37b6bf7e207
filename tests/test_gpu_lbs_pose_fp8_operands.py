"""GPU: the e4m3 form of the SMPL stream kernel's pose phase (description ``SmplF8`` of ``csrc/k2b_lbs_stream.hip``,
``csrc/k2b_lbs_fp8.h``) held to a float64 evaluation of ITS OWN operands: X read back from the model's workspace
(``k2b_dev_lbs_read_x``) and the packed Pd image of ``k2b_dev_lbs_pose_fp8_image``, the builder ``k2b_model_create`` runs.  What
the end-to-end gate of 5e-6 m cannot see - a dropped correction block, a scale one binade off, the wrong half of a lane's 32
bytes, a k-step paired with the wrong strip - moves an output here by at least ``SIGNAL_MIN`` = 3.3e-6 m, or half of it for half
a binade of scale (``tests/test_lbs_pose_fp8_conditions.py``), against a gate of 1e-7 to 2e-7 m.

Layouts (J, NB): (23, 10), (24, 10), (24, 15), (23, 24) - the three ``F8`` instantiations of the pose set-up, ``<32, 3, true>``
included; (24, 15) and (23, 24) fill all 224 k columns.  V = 333, B = 37.  Each layout has the default model and its
``K2B_LBS_POSE_F16=1`` twin.

1. The device encoder ``x_fp8_codes_device`` against the host's ``x_fp8_codes``, code for code, on the X the kernels wrote.
   Saturation cannot be reached through ``k2b_lbs``: the features with codes are entries of R - I, at most 2 in magnitude against
   the limit 28 of X_hi8 (and X_lo <= 2^-11 X_hi against the same limit of X_lo8); the clamp is left to the host tests
   (``tests/test_lbs_pose_fp8_host.py``).
2. The kernel against its operands on the probe models of ``lbs_pose_fp8_common.probe_consts`` (template, shape directions and
   joint regressor zero: all magnitudes are those of the pose correctives), in two skinnings: "blended" (the synthetic weights and
   rotations) and "rigid" (every vertex on the resting root: the transform phase multiplies by exact ones and zeros, the output is
   v_posed).  E8 = skin64(emulate(device X, host image)) for the default model, E16 for the twin.  The gate is not fixed in
   advance: per frame f, r16_f = max|twin - E16| is the floor that the unchanged ``Smpl`` kernel leaves on the same model and
   inputs, the e4m3 form is held to 4 r16_f (the factor ``tests/lbs_backward_common.py`` allows for another summation order), and
   4 r16_f <= SIGNAL_MIN / 16 is asserted so that the gate cannot grow into the signal - on every frame of the rigid models, on
   every frame but the one at 20 rad of the blended ones (a float32 angle of 20 rad is uncertain by 4e-6 rad, which the blended
   transforms turn into 1e-7 m; that frame is held to its own floor all the same).  Vertices, the five vertex-selected joints,
   the kinematic joints, and the joints-only call (the extra set with the mesh's scales) are all held to it.  The "outlier" kinds
   put one coordinate of one vertex at 1 m and at 50 m: that vertex is held apart from the rest to 4 times its own r16 (the
   largest over the frames: three numbers per frame make no floor), without the condition on the signal.
3. One case on the full synthetic model (24, 10), with template and shape, without translation: the same 4 r16 gate; the ratio
   of that gate to SIGNAL_MIN is printed, not asserted (coordinates are 1 m there: it shows how much sharper the probe is).

RESULTS (MI355X; the largest r16_f over the frames under the condition and the e4m3 form's residual there, metres; the outlier
models read the same r16 as dense, their vertices but one being the same):
    layout   rigid: r16      e4m3     gate = SIGNAL_MIN /    blended: r16   e4m3     gate = SIGNAL_MIN /
    23/10    2.33e-8         1.65e-8  35                     3.48e-8        3.17e-8  24
    24/10    2.28e-8         2.12e-8  36                     2.89e-8        3.00e-8  29
    24/15    2.27e-8         1.92e-8  36                     5.10e-8        4.51e-8  16
    23/24    2.63e-8         1.99e-8  31                     3.73e-8        3.77e-8  22
  "step k" models: r16 0.5-1.5e-8 (blended).  Frame at 20 rad, blended: r16 0.7-1.1e-7, e4m3 form 0.6-1.1e-7.  The e4m3 form's
  residual of a frame is at most 1.8 times the twin's.  The floor is not the 1e-9 m a first estimate gave: the rigid models show
  that 2.3e-8 m is the pose phase's own fp32 accumulator (21 MFMAs into sums of 25 in units of Pd x 256: an ulp is 7e-9 m), and
  the blended transforms (fp32 rotations, 22-bit f16 pairs) add as much again.
  Full synthetic model 24/10: r16 7.2e-7, e4m3 form 6.9e-7, gate = SIGNAL_MIN / 1.1.
  Encoder: equal code for code on all four layouts; xh of the two instantiations differs in 0 of 14336 entries."""
import os

import numpy as np
import pytest
import torch

from keypoints2body_amd import native
from tests import helpers as H
from tests import lbs_layouts_common as L
from tests import lbs_pose_fp8_common as P

pytestmark = pytest.mark.gpu

SWITCH = "K2B_LBS_POSE_F16"
ORDER_FACTOR = 4.0
B = P.PROBE_FRAMES
NAN_FRAME, NAN_JOINT = 7, 5


def _native(c, monkeypatch=None):
    make = lambda: native.NativeModel(c.v_template, c.shapedirs, c.posedirs, c.J_regressor, c.lbs_weights, c.parents, c.extra_vertex_ids)
    assert SWITCH not in os.environ
    if monkeypatch is None:
        return make()
    with monkeypatch.context() as mp:
        mp.setenv(SWITCH, "1")
        return make()


def _lbs(model, p, want_vertices=True):
    go, pose, shape, tr = p
    j, v = model.lbs(H.cuda(go), H.cuda(pose), H.cuda(shape), None if tr is None else H.cuda(tr), want_vertices=want_vertices)
    torch.cuda.synchronize()
    return j.double().cpu().numpy(), None if v is None else v.double().cpu().numpy()


def _read_x(model):
    return model.dev_read_x(P.x_halfs(B)[0])


# ---- 1. the encoder, code for code ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("J,NB", P.PROBE_LAYOUTS)
def test_device_encoder_equals_the_host_encoder_code_for_code(J, NB, monkeypatch):
    c = P.probe_consts(J, NB, kind="dense")
    p = P.probe_params(J, NB)
    model, twin = _native(c), _native(c, monkeypatch)
    _lbs(model, p)
    _lbs(twin, p)
    (xh8, xl8), (xh16, xl16) = _read_x(model), _read_x(twin)
    hi, lo, hi8, lo8 = P.unpack_x(xh8, xl8, B, True, padded=True)
    hi_t, lo_t, none_a, none_b = P.unpack_x(xh16, xl16, B, False, padded=True)
    assert not none_a.any() and not none_b.any() and np.isnan(lo[:, :P.CUT]).all() and not np.isnan(lo_t[:B]).any()
    # both instantiations evaluate the same fp32 source: the hi terms are the same bits
    at = P.x_index(B, padded=True)
    differ = xh8[at] != xh16[at]
    print(f"{J}/{NB}: xh of the two models differs in {int(differ.sum())} of {differ.size} entries (left out of the X_lo8 comparison)")
    assert differ.mean() <= 0.01, "the two instantiations of the pose set-up evaluate the features differently"
    # X_hi8 from the model's own hi, X_lo8 from the twin's lo; the host's encoder and the independent one
    live = np.zeros_like(differ)
    live[:B, :P.CUT] = True
    want_hi8, want_lo8 = P._encode(hi[:, :P.CUT], P.X_HI_EXP), P._encode(lo_t[:, :P.CUT], P.X_LO_EXP)
    assert np.array_equal(want_hi8, P._np_encode(hi[:, :P.CUT] / 2.0 ** P.X_HI_EXP)) and np.array_equal(want_lo8, P._np_encode(lo_t[:, :P.CUT] / 2.0 ** P.X_LO_EXP))
    bad_hi = (hi8[:, :P.CUT] != want_hi8) & live[:, :P.CUT]
    bad_lo = (lo8[:, :P.CUT] != want_lo8) & live[:, :P.CUT] & ~differ[:, :P.CUT]
    assert not bad_hi.any(), f"{int(bad_hi.sum())} X_hi8 codes differ from the host's, first at (frame, feature) {np.argwhere(bad_hi)[0]}"
    assert not bad_lo.any(), f"{int(bad_lo.sum())} X_lo8 codes differ from the host's, first at (frame, feature) {np.argwhere(bad_lo)[0]}"
    # the codes the comparison ran over: subnormal, zero and normal ones of X_lo8, and X_hi = -2
    mag = lo8[P.FRAME_LADDER, :63] & 0x7f
    assert ((mag != 0) & (mag < 8)).any() and (mag == 0).any() and (mag >= 8).any()
    assert (hi[P.FRAME_PI, :9 * (J - 1)] == -2.0).sum() == 2 * (J - 1)
    # k-step 6 keeps the f16 form: its lo pieces are the twin's bit for bit
    first = 2 * P.F8_STEPS * P.x_halfs(B)[1] * 16
    assert np.array_equal(xl8[first:], xl16[first:])
    # the padding frames hold zero codes (and zero terms)
    assert not hi8[B:].any() and not lo8[B:].any() and not xh8[at[B:]].any() and not xl8[at[B:]].any()

    # a NaN in one joint of one frame stays in its frame, and its codes are NaN codes
    go, pose, shape, tr = p
    pose_nan = pose.copy()
    pose_nan[NAN_FRAME, 3 * (NAN_JOINT - 1) + 1] = np.nan
    _lbs(model, (go, pose_nan, shape, tr))
    xh_n, xl_n = _read_x(model)
    hi_n, _, hi8_n, lo8_n = P.unpack_x(xh_n, xl_n, B, True)
    nan_at = np.isnan(hi_n[NAN_FRAME, :P.CUT])
    assert nan_at[9 * (NAN_JOINT - 1):9 * NAN_JOINT].any() and nan_at.sum() == nan_at[9 * (NAN_JOINT - 1):9 * NAN_JOINT].sum()
    assert (hi8_n[NAN_FRAME, :P.CUT][nan_at] & 0x7f == 0x7f).all() and (lo8_n[NAN_FRAME, :P.CUT][nan_at] & 0x7f == 0x7f).all()
    others = np.arange(at.shape[0]) != NAN_FRAME
    assert np.array_equal(xh_n[at[others]], xh8[at[others]]) and np.array_equal(xl_n[at[others]], xl8[at[others]])
    clean = ~nan_at
    assert np.array_equal(hi8_n[NAN_FRAME, :P.CUT][clean], hi8[NAN_FRAME, :P.CUT][clean]) and np.array_equal(lo8_n[NAN_FRAME, :P.CUT][clean], lo8[NAN_FRAME, :P.CUT][clean])


# ---- 2. the kernel against its operands -----------------------------------------------------------------------------------------
def _residuals(c, p, model, fp8):
    """name -> |device - E| [B][rows][3] of one model: E from the X the call left in the workspace and the host-built image."""
    J, V = c.parents.shape[0], c.v_template.shape[0]
    ids = c.extra_vertex_ids.astype(np.int64)
    blend = P.blend64(c, p)
    spd, info = P._image(0 if fp8 else 1, consts=c)
    assert bool(info[0]) == fp8
    exps = (int(info[2]), int(info[3]))
    j, v = _lbs(model, p)
    x_ops = P.unpack_x(*_read_x(model), B, fp8)
    ev, ej = P.skin64(c, p, P.emulate(x_ops, P._unpack(spd, info, V), exps, fp8), blend)
    out = {"vertices": np.abs(v - ev), "kinematic joints": np.abs(j[:, :J] - ej), "extra joints": np.abs(j[:, J:] - ev[:, ids])}
    # the joints-only call: the extra set's own image, with the mesh's scales
    j2, none = _lbs(model, p, want_vertices=False)
    assert none is None
    x_ops2 = P.unpack_x(*_read_x(model), B, fp8)
    spd_e, info_e = P._image(0 if fp8 else 1, ids=ids, given=exps if fp8 else None, consts=c)
    assert (int(info_e[2]), int(info_e[3])) == exps
    sub = (blend[0][:, ids], blend[1][:, ids], blend[2])
    ev2, ej2 = P.skin64(c, p, P.emulate(x_ops2, P._unpack(spd_e, info_e, len(ids)), exps, fp8), sub)
    out["joints only: kinematic joints"] = np.abs(j2[:, :J] - ej2)
    out["joints only: extra joints"] = np.abs(j2[:, J:] - ev2)
    assert all(np.isfinite(r).all() for r in out.values())
    return out


def _where(r):
    f, row, coord = np.unravel_index(r.argmax(), r.shape)
    per_frame = r.max(axis=(1, 2))
    worst = np.argsort(per_frame)[::-1][:4]
    return (f"largest at frame {f}, row {row}, coordinate {coord}; per coordinate {r.max(axis=(0, 1))}; worst frames "
            + ", ".join(f"{int(i)}: {per_frame[i]:.2e}" for i in worst))


def _per_frame(r):
    return r.reshape(r.shape[0], -1).max(axis=1)


def _hold(c, p, what, monkeypatch, apart=None, condition=16.0, frames=P.SHARP_FRAMES):
    """Per frame f: r16_f = the twin's largest residual, the gate 4 r16_f, and the e4m3 form's residuals against it.  Asserted on the
    frames of ``SHARP_FRAMES`` - those on which SIGNAL_MIN is read -: 4 r16_f <= SIGNAL_MIN / 16.  (The frame at 20 rad is held to its
    own floor like every other, but a float32 angle of 20 rad is uncertain by 4e-6 rad, which the transforms turn into 1e-7 m.)
    `apart`: a vertex row held to its own floors, apart from the rest and without the condition."""
    r8 = _residuals(c, p, _native(c), True)
    r16 = _residuals(c, p, _native(c, monkeypatch), False)
    groups = {"": {k: (r8[k], r16[k]) for k in r8}}
    if apart is not None:
        rest = np.arange(c.v_template.shape[0]) != apart
        groups[""]["vertices"] = (r8["vertices"][:, rest], r16["vertices"][:, rest])
        groups[f" vertex {apart}"] = {"vertices": (r8["vertices"][:, [apart]], r16["vertices"][:, [apart]])}
    failures = []
    for tag, parts in groups.items():
        floor = np.max([_per_frame(b) for _, b in parts.values()], axis=0)                  # [B]
        if tag:                                            # three numbers per frame: the largest over the frames, not a floor per frame
            floor = np.full_like(floor, floor.max())
        gate = ORDER_FACTOR * floor
        worst = np.max([_per_frame(a) for a, _ in parts.values()], axis=0)
        sharp = float(gate[frames].max())
        print(f"{what}{tag}: r16 {floor[frames].max():.3e} m (frame at 20 rad: {floor[P.FRAME_20RAD]:.3e}), gate 4 r16 = SIGNAL_MIN / "
              f"{P.SIGNAL_MIN / max(sharp, 1e-300):.0f}, e4m3 form {worst[frames].max():.3e} m ({worst[P.FRAME_20RAD]:.3e}), largest e4m3 / r16 of a frame "
              f"{np.max(worst / np.maximum(floor, 1e-300)):.2f}  (" + ", ".join(f"{k} {float(a.max()):.2e} / {float(b.max()):.2e}" for k, (a, b) in parts.items()) + ")")
        if condition and tag == "":
            assert sharp <= P.SIGNAL_MIN / condition, (f"{what}: the floor of the f16 twin, r16 = {sharp / ORDER_FACTOR:.3e} m in frame {int(np.argmax(np.where(frames, gate, 0)))}, "
                                                       f"lets the gate grow into the signal ({P.SIGNAL_MIN:.1e} m / {condition:g})")
        for k, (a, _) in parts.items():
            over = _per_frame(a) > gate
            if over.any():
                f = int(np.argmax(_per_frame(a) / np.maximum(gate, 1e-300)))
                failures.append(f"{what}{tag}, {k}: frame {f} is off its own operands by {_per_frame(a)[f]:.3e} m, gate 4 r16 = {gate[f]:.3e} m ({int(over.sum())} frames over); {_where(a)}")
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("skinning", ("rigid", "blended"))
@pytest.mark.parametrize("kind", P.PROBE_KINDS)
@pytest.mark.parametrize("J,NB", P.PROBE_LAYOUTS)
def test_kernel_computes_what_its_operands_say(J, NB, kind, skinning, monkeypatch):
    rigid = skinning == "rigid"
    c = P.probe_consts(J, NB, kind=kind, rigid=rigid)
    apart = P.outlier_entry(J, NB)[1] // 3 if kind in P.OUTLIER_FACTOR else None
    if rigid:
        _hold(c, P.probe_params(J, NB, rigid=True), f"{J}/{NB} {kind} rigid", monkeypatch, apart=apart, frames=np.ones(B, dtype=bool))
    else:
        _hold(c, P.probe_params(J, NB), f"{J}/{NB} {kind} blended", monkeypatch, apart=apart)


def test_full_synthetic_model_against_its_operands(monkeypatch):
    """(24, 10) with template and shape, without translation: coordinates of 1 m, so the floor r16 - and with it the gate - is that
    of fp32 sums at 1 m; the ratio to SIGNAL_MIN is printed, not asserted."""
    J, NB = 24, 10
    _hold(L.consts(J, NB), P.probe_params(J, NB), f"{J}/{NB} full synthetic model", monkeypatch, condition=None)
