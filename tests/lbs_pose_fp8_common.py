"""Shared by the tests of the e4m3 form of the SMPL stream kernel's pose phase (``csrc/k2b_lbs_fp8.h``, description ``SmplF8`` of
``csrc/k2b_lbs_stream.hip``): ``tests/test_lbs_pose_fp8_host.py``, ``tests/test_lbs_pose_fp8_conditions.py`` and
``tests/test_gpu_lbs_pose_fp8_operands.py``.  Importable without a GPU.

* an independent e4m3fn encoder and decoder, and the development entries of the library (no device needed);
* the two operand layouts written a second time: ``_unpack`` (the packed Pd image) and ``unpack_x`` (the X workspace);
* ``emulate``: ``v_posed`` in float64 from exactly those operands, product by product as the kernel forms them;
* probe models (``probe_consts``) on which nothing but the pose phase contributes an error of the size of one correction block,
  their parameters (``probe_params``) and the float64 skinning of an emulated ``v_posed`` (``skin64``)."""
import ctypes as C
import dataclasses
import functools

import numpy as np

from keypoints2body_amd import native, synthetic

F8_STEPS = 6            # 32-deep k-steps with e4m3 strips; k-step 6 keeps the f16 form
PD_SCALE = 256.0
X_HI_EXP, X_LO_EXP = -4, -15
CUT = 32 * F8_STEPS     # features below it have codes
K_COLS = 224            # k columns of the stream kernel: 7 k-steps of 32

# The smallest contribution, in metres, that ``tests/test_lbs_pose_fp8_conditions.py`` reads for one of the 24 pieces (X_hi8 . Pd_lo8
# and X_lo8 . Pd_hi8 of a k-step 0..5, one 16-feature half each) on some skinned output of the frames SHARP_FRAMES, over the probe
# models, both skinnings and the layouts below: 3.32e-6 m, rounded down.  (Halving a piece's scale moves the same output by half of
# its contribution - the emulation is linear in a scale -, so the second figure of that file is SIGNAL_MIN / 2 = 1.66e-6 m and
# not a figure of its own.)  The probe's posedirs are the synthetic ones, unscaled (factor 1).  That file asserts that no piece
# reads less.
SIGNAL_MIN = 3.3e-6
PROBE_LAYOUTS = ((23, 10), (24, 10), (24, 15), (23, 24))
PROBE_KINDS = ("dense",) + tuple(f"step {k}" for k in range(7)) + ("outlier", "outlier deep")
PROBE_FRAMES = 37
FRAME_ZERO, FRAME_LADDER, FRAME_2RAD, FRAME_PI, FRAME_20RAD = 1, 2, 3, 4, 5   # the special frames of ``probe_params``
SHARP_FRAMES = np.arange(PROBE_FRAMES) != FRAME_20RAD     # the frames on which SIGNAL_MIN is read and the gate must stay below it
OUTLIER_FACTOR = {"outlier": 64.0, "outlier deep": 4096.0}


# ---- an independent encoder ---------------------------------------------------------------------------------------------------
def _decode_table():
    c = np.arange(256)
    e, m = (c >> 3) & 15, c & 7
    mag = np.where(e == 0, m * 2.0 ** -9, (1 + m / 8.0) * 2.0 ** (e.astype(np.float64) - 7))
    mag[(e == 15) & (m == 7)] = np.nan
    return np.where(c & 0x80, -mag, mag)


def _np_encode(x):
    """Nearest finite e4m3fn value, ties to the even code, saturating at +-448; NaN -> 0x7f | sign."""
    x = np.asarray(x, dtype=np.float64)
    mags = _decode_table()[:0x7f]                              # codes 0..0x7e: increasing magnitudes 0..448
    a = np.minimum(np.abs(x), 448.0)
    hi = np.clip(np.searchsorted(mags, a), 1, 0x7e)            # first code with magnitude >= a
    lo = hi - 1
    dlo, dhi = a - mags[lo], mags[hi] - a
    code = np.where(dlo < dhi, lo, np.where(dhi < dlo, hi, np.where(lo % 2 == 0, lo, hi)))
    code = np.where(np.isnan(x), 0x7f, code).astype(np.uint8)
    return code | (np.signbit(x).astype(np.uint8) << 7)


def _lib():
    return native.load_library()


def _encode(x, exp=0):
    x = np.ascontiguousarray(x, dtype=np.float32)
    out = np.empty(x.size, dtype=np.uint8)
    fn = _lib().k2b_dev_e4m3_encode
    fn.restype = C.c_int
    rc = fn(C.c_int64(x.size), x.ctypes.data_as(C.c_void_p), C.c_int32(exp), out.ctypes.data_as(C.c_void_p))
    assert rc == 0
    return out.reshape(x.shape)


# ---- the images -----------------------------------------------------------------------------------------------------------------
_memo = {}


def _consts():
    if "c" not in _memo:
        _memo["c"] = synthetic.make_body_model(0)
    return _memo["c"]


def _ids():
    return np.sort(np.random.default_rng(2).choice(_consts().v_template.shape[0], 1000, replace=False)).astype(np.int32)


def _image(pose_f16, ids=None, given=None, consts=None):
    """(spd as uint16, info = [pose_fp8, nv16, lo_exp, hi_exp]) of the vertex set `ids` of the synthetic model, or of the model
    `consts` (then `ids` = None is the whole mesh, the set whose scales ``k2b_model_create`` takes)."""
    c = _consts() if consts is None else consts
    if ids is None:
        ids = _ids() if consts is None else np.arange(c.v_template.shape[0])
    ids = np.ascontiguousarray(ids, dtype=np.int32)
    V, J, NB = c.v_template.shape[0], c.parents.shape[0], c.shapedirs.shape[-1]
    f = lambda a: np.ascontiguousarray(a, dtype=np.float32)
    arrs = [f(c.v_template), f(c.shapedirs), f(c.posedirs), f(c.lbs_weights)]
    fn = _lib().k2b_dev_lbs_pose_fp8_image
    fn.restype = C.c_int
    n, info = C.c_int64(0), np.zeros(4, dtype=np.int32)
    gv = None if given is None else np.asarray(given, dtype=np.int32)
    head = [C.c_int32(J), C.c_int32(NB), C.c_int32(V), C.c_int32(len(ids)), ids.ctypes.data_as(C.c_void_p)] + \
           [a.ctypes.data_as(C.c_void_p) for a in arrs] + [C.c_int32(pose_f16), None if gv is None else gv.ctypes.data_as(C.c_void_p)]
    assert fn(*head, None, C.byref(n), info.ctypes.data_as(C.c_void_p)) == 0
    spd = np.zeros(n.value, dtype=np.uint16)
    assert fn(*head, spd.ctypes.data_as(C.c_void_p), C.byref(n), info.ctypes.data_as(C.c_void_p)) == 0
    return spd, info


def _unpack(spd, info, n):
    """The layout, a second time.  spd [k-step 7][16-vertex tile][coordinate 3][hi | lo] in 1 KiB pieces.  f16 piece: lane =
    vertex row + 16 * (k >> 3) holds 8 halfs k & 7.  e4m3 piece (k-steps 0..5 of a pose_fp8 image, in place of lo): lane group g
    (16 bytes per lane, lane = row + 16 g) = Pd_lo8[k 0..15], Pd_lo8[k 16..31], Pd_hi8[k 0..15], Pd_hi8[k 16..31].
    Returns hi, lo (f16 terms as float64, lo NaN where the image has codes), lo8, hi8 (codes, 0 where none): [224][n][3]."""
    fp8, nv16 = int(info[0]), int(info[1])
    pieces = spd.reshape(7, nv16, 3, 2, 512)
    halfs, raw = pieces.view(np.float16), pieces.view(np.uint8).reshape(7, nv16, 3, 2, 1024)
    i = np.arange(n)
    v16, r = i >> 4, i & 15
    k = np.arange(224)
    ks, kk = k >> 5, k & 31
    at16 = ((kk >> 3)[:, None] * 16 + r[None, :]) * 8 + (kk & 7)[:, None]                      # [k][vertex]
    hi = np.stack([halfs[ks[:, None], v16[None, :], c, 0, at16] for c in range(3)], axis=-1).astype(np.float64)
    lo = np.stack([halfs[ks[:, None], v16[None, :], c, 1, at16] for c in range(3)], axis=-1).astype(np.float64)
    lo8 = np.zeros((224, n, 3), dtype=np.uint8)
    hi8 = np.zeros_like(lo8)
    if fp8:
        at_lo8 = ((kk >> 4)[:, None] * 16 + r[None, :]) * 16 + (kk & 15)[:, None]
        at_hi8 = ((2 + (kk >> 4))[:, None] * 16 + r[None, :]) * 16 + (kk & 15)[:, None]
        lo8 = np.stack([raw[ks[:, None], v16[None, :], c, 1, at_lo8] for c in range(3)], axis=-1)
        hi8 = np.stack([raw[ks[:, None], v16[None, :], c, 1, at_hi8] for c in range(3)], axis=-1)
        lo[: 32 * F8_STEPS] = np.nan
        lo8[32 * F8_STEPS:] = 0
        hi8[32 * F8_STEPS:] = 0
    return hi, lo, lo8, hi8


def frag_elem(frag, k, row):
    """``frag_elem`` of ``csrc/k2b_layout.h``: element (k of a 16-deep k-step, row of a 32-row tile) of piece number `frag`."""
    return ((frag * 2 + ((k >> 3) & 1)) * 32 + (row & 31)) * 8 + (k & 7)


def x_halfs(B):
    """(halfs of the X workspace of a B-frame call on the stream route, padded frames)."""
    bpad = (B + 31) // 32 * 32
    return (K_COLS // 16) * bpad * 16, bpad


def x_index(B, padded=False):
    """[B or padded frames][224]: where the half of (frame, feature) stands in xh and in xl; a frame's 224 positions are all it
    owns of either array (its 28 16-byte chunks)."""
    _, bpad = x_halfs(B)
    f = np.arange(bpad if padded else B)[:, None]
    K = np.arange(K_COLS)[None, :]
    return frag_elem((K >> 4) * (bpad // 32) + (f >> 5), K & 15, f)


def unpack_x(xh, xl, B, fp8, padded=False):
    """The layout of X, a second time.  xh, xl: uint16 [14 x padded frames x 16], pieces [16-deep k-step 14][32-frame tile] of
    ``frag_elem`` order (tiles = padded frames / 32).  For an fp8 model the lo pieces of the 32-deep k-steps s = 0..5 hold, per frame
    and in place of the four 8-half chunks (16-deep k-step 2 s + (g >> 1), k half g & 1) of the lane groups g = 0..3, the 16-byte
    chunks X_hi8[0..15] | X_hi8[16..31] | X_lo8[0..15] | X_lo8[16..31] of k-step s (``put_x`` and the store loop of
    ``k2b_pose_setup_kernel``).  Returns hi, lo (float64, lo NaN where codes are), hi8, lo8 (codes, 0 where none): [B][224], or
    with `padded` the rows of the padding frames as well."""
    halfs, bpad = x_halfs(B)
    assert xh.shape == (halfs,) and xl.shape == (halfs,) and xh.dtype == np.uint16 and xl.dtype == np.uint16
    tiles = bpad // 32
    at = x_index(B, padded)
    B = at.shape[0]
    f = np.arange(B)[:, None]
    hi = xh.view(np.float16)[at].astype(np.float64)
    lo = xl.view(np.float16)[at].astype(np.float64)
    hi8 = np.zeros((B, K_COLS), dtype=np.uint8)
    lo8 = np.zeros_like(hi8)
    if fp8:
        raw = xl.view(np.uint8)
        Kc = np.arange(CUT)[None, :]
        s, kk = Kc >> 5, Kc & 31
        for codes, first in ((hi8, 0), (lo8, 2)):
            g = first + (kk >> 4)
            chunk = frag_elem((2 * s + (g >> 1)) * tiles + (f >> 5), 8 * (g & 1), f)             # first half of the 16-byte chunk
            codes[:, :CUT] = raw[2 * chunk + (kk & 15)]
        lo[:, :CUT] = np.nan
    return hi, lo, hi8, lo8


# ---- the arithmetic of the pose phase -------------------------------------------------------------------------------------------
def emulate(x_ops, pd_ops, exps, fp8):
    """v_posed [B][n][3] in float64 from the operands themselves.  x_ops = (hi, lo, hi8, lo8) [B][224], pd_ops = (hi, lo, lo8, hi8)
    [224][n][3] (``_unpack``'s order), exps = (pd8_lo_exp, pd8_hi_exp).  The hi product over all 7 k-steps; then either the two
    f16 corrections of every k-step, or - fp8 - those of k-step 6 and, for the k-steps 0..5, the decoded codes with their four
    scales: X_hi8 2^-4 . Pd_lo8 2^lo_exp + X_lo8 2^-15 . Pd_hi8 2^hi_exp.  In units of Pd x 256, divided at the end."""
    xh, xl, xh8, xl8 = x_ops
    hi, lo, lo8, hi8 = pd_ops
    dec = _decode_table()
    cut = CUT
    acc = np.einsum("bk,kvc->bvc", xh, hi)
    if not fp8:
        acc += np.einsum("bk,kvc->bvc", xh, lo) + np.einsum("bk,kvc->bvc", xl, hi)
    else:
        acc += np.einsum("bk,kvc->bvc", xh[:, cut:], lo[cut:]) + np.einsum("bk,kvc->bvc", xl[:, cut:], hi[cut:])
        a_hi, a_lo = dec[xh8[:, :cut]] * 2.0 ** X_HI_EXP, dec[xl8[:, :cut]] * 2.0 ** X_LO_EXP
        b_lo, b_hi = dec[lo8[:cut]] * 2.0 ** int(exps[0]), dec[hi8[:cut]] * 2.0 ** int(exps[1])
        acc += np.einsum("bk,kvc->bvc", a_hi, b_lo) + np.einsum("bk,kvc->bvc", a_lo, b_hi)
    return acc / PD_SCALE


PIECES = tuple((prod, s, h) for prod in ("hi8.lo8", "lo8.hi8") for s in range(F8_STEPS) for h in range(2))


def piece(x_ops, pd_ops, exps, which):
    """The share of ``emulate``'s e4m3 sum that one of PIECES contributes: which = (product, k-step, 16-feature half)."""
    prod, s, h = which
    _, _, xh8, xl8 = x_ops
    _, _, lo8, hi8 = pd_ops
    dec = _decode_table()
    k = slice(32 * s + 16 * h, 32 * s + 16 * h + 16)
    if prod == "hi8.lo8":
        a, b = dec[xh8[:, k]] * 2.0 ** X_HI_EXP, dec[lo8[k]] * 2.0 ** int(exps[0])
    else:
        a, b = dec[xl8[:, k]] * 2.0 ** X_LO_EXP, dec[hi8[k]] * 2.0 ** int(exps[1])
    return np.einsum("bk,kvc->bvc", a, b) / PD_SCALE


# ---- features -------------------------------------------------------------------------------------------------------------------
def _rot_minus_identity(aa):
    """R - I [..., 3, 3] in float64 of the rotation vectors aa [..., 3]."""
    th = np.linalg.norm(aa, axis=-1, keepdims=True)
    ax = aa / np.maximum(th, 1e-300)
    K = np.zeros(aa.shape[:-1] + (3, 3))
    K[..., 0, 1], K[..., 0, 2], K[..., 1, 0] = -ax[..., 2], ax[..., 1], ax[..., 2]
    K[..., 1, 2], K[..., 2, 0], K[..., 2, 1] = -ax[..., 0], -ax[..., 1], ax[..., 0]
    s, c1 = np.sin(th)[..., None], (1 - np.cos(th))[..., None]
    return s * K + c1 * (K @ K)


def _features(pose, betas):
    """X [B][224] in float64 from float32 parameters: vec(R_j - I) of the 23 body joints (row-major), betas, 1, 1, zeros."""
    B = pose.shape[0]
    aa = pose.astype(np.float64).reshape(B, 23, 3)
    RmI = _rot_minus_identity(aa)
    X = np.zeros((B, 224))
    X[:, :207] = RmI.reshape(B, 207)
    X[:, 207:217] = betas
    X[:, 217:219] = 1.0
    return X


def features(J, NB, p):
    """``_features`` for J joints and NB coefficients: p = (global_orient, pose, shape, transl) as ``lbs_layouts_common.params``."""
    _, pose, shape, _ = p
    B, P = pose.shape[0], 9 * (J - 1)
    X = np.zeros((B, K_COLS))
    X[:, :P] = _rot_minus_identity(pose.astype(np.float64).reshape(B, J - 1, 3)).reshape(B, P)
    X[:, P:P + NB] = shape
    X[:, P + NB:P + NB + 2] = 1.0
    return X


def _x_terms(X32):
    x = np.ascontiguousarray(X32, dtype=np.float32).reshape(-1)
    hi, lo = np.empty_like(x), np.empty_like(x)
    hi8, lo8 = np.empty(x.size, dtype=np.uint8), np.empty(x.size, dtype=np.uint8)
    fn = _lib().k2b_dev_lbs_x_fp8
    fn.restype = C.c_int
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    assert fn(C.c_int64(x.size), p(x), p(hi), p(lo), p(hi8), p(lo8)) == 0
    sh = X32.shape
    return hi.reshape(sh).astype(np.float64), lo.reshape(sh).astype(np.float64), hi8.reshape(sh), lo8.reshape(sh)


# ---- probe models ---------------------------------------------------------------------------------------------------------------
def outlier_entry(J, NB, V=333):
    """(posedirs row = feature, column = 3 vertex + coordinate) of the entry the "outlier" kinds enlarge: the largest of the
    k-steps 0..5."""
    from tests import lbs_layouts_common as L
    pd = L.consts(J, NB, V).posedirs[:CUT]
    return tuple(int(i) for i in np.unravel_index(np.abs(pd).argmax(), pd.shape))


@functools.lru_cache(maxsize=None)
def probe_consts(J, NB, V=333, kind="dense", rigid=False):
    """``lbs_layouts_common.consts(J, NB, V)`` with v_template, shapedirs and J_regressor set to zero: every joint sits at the
    origin, the transforms are pure rotations, and without translation the output is sum_j w_vj G_j v_posed - all magnitudes are
    those of the pose correctives, a few centimetres, so the fp32 and f16-split roundings of everything behind the pose phase fall
    to about 1e-9 m while a correction block keeps its size.  `kind`: "dense" (the synthetic posedirs), "step k" (k = 0..6: the
    posedirs of the features outside the 32-deep k-step k zeroed, so that a failure names the k-step), "outlier" and "outlier
    deep" (dense with the largest entry of the k-steps 0..5 multiplied by 64 and by 4096: the image's hi scale rises by six and
    by twelve binades, the lo scale by five and eleven; at 64 one Pd_lo8 code in fifty is an e4m3 subnormal, at 4096 half of
    them are and one in twelve is zero - the form is inaccurate there by design, and must still compute what its operands say).
    The enlarged entry puts one coordinate of one vertex (``outlier_entry``) at 1 m and at 50 m: the tests hold that vertex apart.
    `rigid`: every vertex hangs on the root alone (weight 1); with the root at rest (``probe_params(..., rigid=True)``) the
    transform phase multiplies by exact ones and zeros, the output IS v_posed, and the only roundings left are those of the pose
    phase's fp32 accumulator, some 1e-9 m.  (With the blended weights the transform phase leaves 3e-7 of v_posed - fp32
    rotations, 22-bit f16 pairs -, 3e-8 m: measured, ``tests/test_gpu_lbs_pose_fp8_operands.py``.)"""
    from tests import lbs_layouts_common as L
    c = L.consts(J, NB, V)
    pd = c.posedirs.copy()
    if kind.startswith("step "):
        k = int(kind.split()[1])
        keep = np.zeros(pd.shape[0], dtype=bool)
        keep[32 * k:32 * k + 32] = True
        pd[~keep] = 0.0
    elif kind in OUTLIER_FACTOR:
        r, col = outlier_entry(J, NB, V)
        pd[r, col] *= np.float32(OUTLIER_FACTOR[kind])
    else:
        assert kind == "dense", kind
    w = c.lbs_weights
    if rigid:
        w = np.zeros_like(w)
        w[:, 0] = 1.0
    return dataclasses.replace(c, v_template=np.zeros_like(c.v_template), shapedirs=np.zeros_like(c.shapedirs),
                               J_regressor=np.zeros_like(c.J_regressor), posedirs=pd, lbs_weights=w)


@functools.lru_cache(maxsize=None)
def probe_params(J, NB, B=PROBE_FRAMES, rigid=False):
    """``lbs_layouts_common.params(J, NB, "wide", B)`` (frame 1 all zero, frame 2 the LADDER angles - down to where X_lo 2^15
    falls into the e4m3 subnormals -, frame 3 at 2 rad) with frame 4 at pi about a coordinate axis on every joint (X_hi = -2
    exactly) and frame 5 at about 20 rad about seeded axes; the translation is None.  `rigid`: the root at rest in every frame (the other joints, and with them X, unchanged)."""
    from tests import lbs_layouts_common as L
    go, pose, shape, _ = (a.copy() for a in L.params(J, NB, "wide", B))
    full = np.concatenate([go, pose], axis=1).reshape(B, J, 3).astype(np.float64)
    rng = np.random.default_rng([J, NB, 2000])
    full[FRAME_PI] = np.pi * np.eye(3)[np.arange(J) % 3]
    d = rng.standard_normal((J, 3))
    full[FRAME_20RAD] = 20.0 * d / np.linalg.norm(d, axis=-1, keepdims=True) * rng.uniform(0.9, 1.1, (J, 1))
    if rigid:
        full[:, 0] = 0.0
    f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)
    return f32(full[:, 0]), f32(full[:, 1:].reshape(B, 3 * (J - 1))), shape, None


def blend64(consts, p):
    """Float64 skinning operands of the float32 parameters p: (M [B][V][3][3] = sum_j w_vj R_j, T [B][V][3] = sum_j w_vj t_j,
    joints [B][J][3]) with A_j = [R_j | t_j] the global transform of joint j relative to its rest position (Rodrigues, chained
    over `parents`; the rest joints from J_regressor, v_template, shapedirs and the shape)."""
    go, pose, shape, _ = p
    B, J = go.shape[0], consts.parents.shape[0]
    aa = np.concatenate([go, pose], axis=1).astype(np.float64).reshape(B, J, 3)
    R = _rot_minus_identity(aa) + np.eye(3)
    v_shaped = consts.v_template.astype(np.float64)[None] + np.einsum("vck,bk->bvc", consts.shapedirs.astype(np.float64), shape.astype(np.float64))
    rest = np.einsum("jv,bvc->bjc", consts.J_regressor.astype(np.float64), v_shaped)
    Rg, pg = np.zeros((B, J, 3, 3)), np.zeros((B, J, 3))
    for j in range(J):
        par = int(consts.parents[j])
        if j == 0 or par < 0:
            Rg[:, j], pg[:, j] = R[:, j], rest[:, j]
        else:
            Rg[:, j] = Rg[:, par] @ R[:, j]
            pg[:, j] = pg[:, par] + np.einsum("bij,bj->bi", Rg[:, par], rest[:, j] - rest[:, par])
    t = pg - np.einsum("bjik,bjk->bji", Rg, rest)
    w = consts.lbs_weights.astype(np.float64)
    return np.einsum("vj,bjik->bvik", w, Rg), np.einsum("vj,bji->bvi", w, t), pg


def skin64(consts, p, v_posed, blend=None):
    """(vertices [B][V][3], kinematic joints [B][J][3]) in float64: the rotations and weights applied to `v_posed` [B][V][3] (the
    translation of p, if any, added); `blend` = ``blend64(consts, p)`` computed before."""
    M, T, joints = blend64(consts, p) if blend is None else blend
    out = np.einsum("bvik,bvk->bvi", M, v_posed) + T
    if p[3] is not None:
        tr = p[3].astype(np.float64)[:, None]
        out, joints = out + tr, joints + tr
    return out, joints
