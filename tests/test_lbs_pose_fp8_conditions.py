"""Host: the conditions that keep ``tests/test_gpu_lbs_pose_fp8_operands.py`` sharp, from the float64 emulation alone
(``tests/lbs_pose_fp8_common.py``): X made on the host by ``k2b_dev_lbs_x_fp8`` from float64 features, the Pd image by
``k2b_dev_lbs_pose_fp8_image``.  No device.

* power: on every probe model and layout each live one of the 24 pieces - X_hi8 . Pd_lo8 and X_lo8 . Pd_hi8 of a k-step 0..5, one
  16-feature half each - contributes at least 1e-6 m to some skinned output, and halving its scale moves some output by at least
  5e-7 m; the smallest contribution is at least ``SIGNAL_MIN``.  (A "step k" model has the four pieces of its k-step; "step 6" has
  none.)
* subnormals: the "outlier deep" image has at least a quarter of its non-zero Pd_lo8 codes subnormal ("outlier", with the factor
  64, has one in fifty: see the test); the LADDER frame has X_lo8 codes both subnormal and zero.
* four emulated mis-maps each move some output by at least ``SIGNAL_MIN / 2``."""
import numpy as np
import pytest

from tests import lbs_pose_fp8_common as P

_memo = {}


def _case(J, NB, kind, rigid=False):
    """(consts, params, x_ops, pd_ops, exps, blend) of one probe model, computed once."""
    key = (J, NB, kind, rigid)
    if key not in _memo:
        c = P.probe_consts(J, NB, kind=kind, rigid=rigid)
        p = P.probe_params(J, NB, rigid=rigid)
        x_ops = P._x_terms(P.features(J, NB, p).astype(np.float32))
        spd, info = P._image(0, consts=c)
        assert info[0] == 1, "the layout is not on the e4m3 form"
        if ("blend", J, NB, rigid) not in _memo:
            _memo[("blend", J, NB, rigid)] = P.blend64(c, p)     # the rotations do not depend on the posedirs
        _memo[key] = (c, p, x_ops, P._unpack(spd, info, c.v_template.shape[0]), (int(info[2]), int(info[3])), _memo[("blend", J, NB, rigid)])
    return _memo[key]


def _skinned(case, v_posed):
    """The skinned share of `v_posed` on the frames the GPU test holds sharply (``SHARP_FRAMES``: all but the one at 20 rad, where
    the float32 angle itself leaves 1e-7 m); linear in v_posed: the joints sit at the origin."""
    c, p, _, _, _, blend = case
    M = blend[0]
    return np.einsum("bvik,bvk->bvi", M, v_posed)[P.SHARP_FRAMES]


def _live(kind):
    if kind.startswith("step "):
        k = int(kind.split()[1])
        return tuple(w for w in P.PIECES if w[1] == k)
    return P.PIECES


@pytest.mark.parametrize("rigid", (False, True))
@pytest.mark.parametrize("kind", P.PROBE_KINDS)
@pytest.mark.parametrize("J,NB", P.PROBE_LAYOUTS)
def test_every_piece_is_visible(J, NB, kind, rigid):
    case = _case(J, NB, kind, rigid)
    _, p, x_ops, pd_ops, exps, blend = case
    assert np.abs(blend[1]).max() == 0.0 and np.abs(blend[2]).max() == 0.0       # pure rotations
    if rigid:
        assert np.array_equal(blend[0], np.broadcast_to(np.eye(3), blend[0].shape))     # and here the identity: the output is v_posed
    base = _skinned(case, P.emulate(x_ops, pd_ops, exps, True))
    figures = {}
    for which in _live(kind):
        share = P.piece(x_ops, pd_ops, exps, which)
        contribution = float(np.abs(_skinned(case, share)).max())
        # halving the piece's scale: the emulation with that one scale a binade down
        halved = float(np.abs(_skinned(case, P.emulate(x_ops, pd_ops, exps, True) - 0.5 * share) - base).max())
        figures[which] = (contribution, halved)
    if not figures:
        return
    low = min(figures, key=lambda w: figures[w][0])
    print(f"{J}/{NB} {kind}{' rigid' if rigid else ''}: smallest piece {low} contributes {figures[low][0]:.2e} m, halved scale moves {figures[low][1]:.2e} m; "
          f"largest {max(f[0] for f in figures.values()):.2e} m; scales {exps}")
    for which, (contribution, halved) in figures.items():
        assert contribution >= 1e-6, (which, contribution)
        assert halved >= 5e-7, (which, halved)
        assert contribution >= P.SIGNAL_MIN and halved >= P.SIGNAL_MIN / 2, (which, contribution, halved, P.SIGNAL_MIN)


def _subnormal_share(codes):
    mag = codes & 0x7f
    return float(((mag != 0) & (mag < 8)).sum() / max(1, (mag != 0).sum())), float((mag == 0).mean())


@pytest.mark.parametrize("J,NB", P.PROBE_LAYOUTS)
def test_subnormal_codes_are_reached(J, NB):
    """The factor 64 that the "outlier" model was first given leaves one Pd_lo8 code in fifty subnormal (the f16 lo terms of the
    image spread over twelve binades below their largest, and e4m3 has nine binades of normal codes below 448 / 2^5): the quarter
    is asserted on "outlier deep", factor 4096, the smallest power of two at which a third, and with it a quarter, is reached
    for all four layouts (2048: 0.34, 4096: 0.52); "outlier" must have some, and more than "dense"."""
    shares = {kind: _subnormal_share(_case(J, NB, kind)[3][2][:P.CUT]) for kind in ("dense", "outlier", "outlier deep")}
    exps = {kind: _case(J, NB, kind)[4] for kind in shares}
    print(f"{J}/{NB}: (subnormal share of the non-zero Pd_lo8 codes, zero share) " + " ".join(f"{k}: {v[0]:.3f}, {v[1]:.3f} scales {exps[k]}" for k, v in shares.items()))
    assert shares["outlier deep"][0] >= 0.25
    assert shares["outlier"][0] > shares["dense"][0] and shares["outlier"][0] > 0.0
    assert exps["outlier"][1] == exps["dense"][1] + 6 and exps["outlier deep"][1] == exps["dense"][1] + 12     # the hi scale: six binades per factor 64
    x_ops = _case(J, NB, "dense")[2]
    x_lo8 = x_ops[3][P.FRAME_LADDER, :9 * 7] & 0x7f               # the joints 1..7 carry the LADDER angles 1e-6 .. 3.3
    assert ((x_lo8 != 0) & (x_lo8 < 8)).any() and (x_lo8 == 0).any(), x_lo8
    x_hi = x_ops[0][P.FRAME_PI, :9 * (J - 1)]
    # pi about a coordinate axis: two diagonal entries of R - I are -2 exactly, the rest sin(float32 pi) = -8.7e-8 at the most
    assert (x_hi == -2.0).sum() == 2 * (J - 1) and np.abs(x_hi[x_hi != -2.0]).max() < 1e-7


def _swap_pairs(a, axis):
    """the 32-deep k-steps 0 <-> 1, 2 <-> 3, 4 <-> 5 of the k axis exchanged"""
    a = np.moveaxis(a.copy(), axis, 0)
    b = a.copy()
    for s in range(0, P.F8_STEPS, 2):
        b[32 * s:32 * s + 32], b[32 * s + 32:32 * s + 64] = a[32 * s + 32:32 * s + 64], a[32 * s:32 * s + 32]
    return np.moveaxis(b, 0, axis)


def _swap_halves(a, axis):
    """the two 16-feature halves of every k-step 0..5 exchanged"""
    a = np.moveaxis(a.copy(), axis, 0)
    b = a.copy()
    for s in range(P.F8_STEPS):
        b[32 * s:32 * s + 16], b[32 * s + 16:32 * s + 32] = a[32 * s + 16:32 * s + 32], a[32 * s:32 * s + 16]
    return np.moveaxis(b, 0, axis)


MISMAPS = ("pd pairs swapped", "blocks 1 and 3", "pd scales swapped", "x lane groups 0 and 1")


def _mismapped(name, x_ops, pd_ops, exps):
    xh, xl, xh8, xl8 = x_ops
    hi, lo, lo8, hi8 = pd_ops
    if name == "pd pairs swapped":          # the even and the odd k-step of a pair exchanged on the Pd side only
        return x_ops, (hi, lo, _swap_pairs(lo8, 0), _swap_pairs(hi8, 0)), exps
    if name == "blocks 1 and 3":            # X_lo8 . Pd_hi8 of the even and of the odd k-step: exchanged on one operand (X) - on
        return (xh, xl, xh8, _swap_pairs(xl8, 1)), pd_ops, exps       # both it is the same sum, the two blocks having the same scales
    if name == "pd scales swapped":
        return x_ops, pd_ops, (exps[1], exps[0])
    if name == "x lane groups 0 and 1":     # X_hi8[0..15] and X_hi8[16..31] of every k-step exchanged, X side only
        return (xh, xl, _swap_halves(xh8, 1), xl8), pd_ops, exps
    raise ValueError(name)


@pytest.mark.parametrize("rigid", (False, True))
@pytest.mark.parametrize("name", MISMAPS)
@pytest.mark.parametrize("kind", ("dense", "outlier", "outlier deep"))
@pytest.mark.parametrize("J,NB", P.PROBE_LAYOUTS)
def test_mis_maps_are_visible_in_the_emulation(J, NB, kind, name, rigid):
    case = _case(J, NB, kind, rigid)
    _, _, x_ops, pd_ops, exps, _ = case
    base = P.emulate(x_ops, pd_ops, exps, True)
    moved = float(np.abs(_skinned(case, P.emulate(*_mismapped(name, x_ops, pd_ops, exps), True) - base)).max())
    print(f"{J}/{NB} {kind}{' rigid' if rigid else ''}: {name} moves {moved:.2e} m ({moved / P.SIGNAL_MIN:.1f} SIGNAL_MIN)")
    assert moved >= P.SIGNAL_MIN / 2, (name, moved)


def test_probe_params_hold_the_special_frames():
    J, NB = 24, 10
    go, pose, shape, tr = P.probe_params(J, NB)
    assert tr is None and go.shape == (P.PROBE_FRAMES, 3) and pose.shape == (P.PROBE_FRAMES, 3 * (J - 1)) and go.dtype == np.float32
    full = np.concatenate([go, pose], axis=1).reshape(P.PROBE_FRAMES, J, 3).astype(np.float64)
    angle = np.linalg.norm(full, axis=-1)
    assert not full[P.FRAME_ZERO].any()
    assert np.allclose(angle[P.FRAME_2RAD], 2.0, atol=1e-6) and np.allclose(angle[P.FRAME_PI], np.pi, atol=1e-6)
    assert (angle[P.FRAME_20RAD] >= 17.9).all() and (angle[P.FRAME_20RAD] <= 22.1).all()
    assert angle[P.FRAME_LADDER, 1] == pytest.approx(1e-6, rel=1e-3)
