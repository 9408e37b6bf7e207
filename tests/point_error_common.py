"""Float64 oracle and seeded case generators of the positional-error tests (``k2b_point_error``: MPJPE / PA-MPJPE / PVE).

The oracle is numpy float64 and knows nothing of the kernel: weighted Umeyama through ``numpy.linalg.svd`` with the determinant
correction (``oracle``), and Horn's quaternion form through ``numpy.linalg.eigh`` (``oracle_horn_err``), which only serves to
show that a case is well conditioned: two unrelated formulations agree on its errors.
"""
import numpy as np

MODES = ("none", "translation", "rigid", "similarity")       # align_mode 0..3
POINT_COUNTS = (1, 2, 3, 4, 22, 63, 64, 65, 255, 256, 257, 1000)
FRAME_COUNTS = (1, 3, 5, 257)
WEIGHT_KINDS = ("none", "shared", "frame")
MESH_POINTS, MESH_FRAMES = 10475, 2


def random_rotation(rng) -> np.ndarray:
    """A proper rotation, uniform enough: the orthogonal factor of a Gaussian matrix with its determinant made +1."""
    q, r = np.linalg.qr(rng.standard_normal((3, 3)))
    q = q * np.sign(np.diag(r))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    return q


def make_case(seed: int, B: int, N: int, weights: str = "none", offset: float = 0.0, noise: float = 0.05):
    """``(pred, gt, w)`` float32: ``pred`` a body-sized cloud (|coordinates| up to about 2 m, thinner along two axes), ``gt`` a
    similarity transform of it per frame plus ``noise``; ``w`` None, ``[N]`` or ``[B][N]`` with about a fifth of the per-frame
    weights zero.  ``offset`` is added to every coordinate of both sets (the centring case)."""
    rng = np.random.default_rng([seed, B, N, WEIGHT_KINDS.index(weights)])
    pred = rng.uniform(-1.0, 1.0, (B, N, 3)) * np.array([1.6, 0.9, 0.5])
    gt = np.empty_like(pred)
    for b in range(B):
        s, R, t = rng.uniform(0.7, 1.4), random_rotation(rng), rng.uniform(-0.4, 0.4, 3)
        gt[b] = s * pred[b] @ R.T + t + noise * rng.standard_normal((N, 3))
    w = None
    if weights == "shared":
        w = rng.uniform(0.2, 2.0, N)
    elif weights == "frame":
        w = rng.uniform(0.2, 2.0, (B, N)) * (rng.uniform(0, 1, (B, N)) > 0.2)
    f32 = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.float32)
    return f32(pred + offset), f32(gt + offset), f32(w)


def frame_scale(pred, gt) -> np.ndarray:
    """``L``: the largest coordinate magnitude of each frame, ``[B]``."""
    B = pred.shape[0]
    return np.maximum(np.abs(pred.reshape(B, -1)).max(1), np.abs(gt.reshape(B, -1)).max(1)).astype(np.float64)


def _frame_weights(w, B, N):
    if w is None:
        return np.ones((B, N))
    w = np.asarray(w, dtype=np.float64)
    return np.broadcast_to(w, (B, N)) if w.ndim == 1 else w


def _coincide(x, w) -> bool:
    live = x[w > 0]
    return live.shape[0] <= 1 or bool(np.all(live == live[0]))


def oracle(pred, gt, w=None, mode: int = 0) -> dict:
    """Per frame in float64: ``err [B]``, ``per_point [B][N]``, ``transform [B][13]`` (s, R row-major, t) and ``gap [B]`` =
    ``(s2 + d s3) / s1`` of the covariance's singular values (0: the rotation is not unique, only the error is; NaN where no
    rotation is sought)."""
    x, y = np.asarray(pred, dtype=np.float64), np.asarray(gt, dtype=np.float64)
    B, N, _ = x.shape
    W = _frame_weights(w, B, N)
    out = dict(err=np.zeros(B), per_point=np.zeros((B, N)), transform=np.zeros((B, 13)), gap=np.full(B, np.nan))
    for b in range(B):
        wb, s, R, t = W[b], 1.0, np.eye(3), np.zeros(3)
        tot = wb.sum()
        if tot == 0:                                           # no weight at all: error 0, identity transform
            out["transform"][b] = np.concatenate([[1.0], np.eye(3).ravel(), np.zeros(3)])
            continue
        if mode >= 1:
            cx, cy = (wb[:, None] * x[b]).sum(0) / tot, (wb[:, None] * y[b]).sum(0) / tot
            if mode >= 2 and _coincide(x[b], wb):
                cx = x[b][wb > 0][0]
            elif mode >= 2:
                dx, dy = x[b] - cx, y[b] - cy
                cov = (wb[:, None] * dy).T @ dx                # sum w (y - cy)(x - cx)^T: R = U D V^T maps x to y
                U, sv, Vt = np.linalg.svd(cov)
                d = 1.0 if np.linalg.det(U) * np.linalg.det(Vt) > 0 else -1.0
                R = U @ np.diag([1.0, 1.0, d]) @ Vt
                out["gap"][b] = (sv[1] + d * sv[2]) / sv[0] if sv[0] > 0 else 0.0
                if mode == 3:
                    s = (sv[0] + sv[1] + d * sv[2]) / (wb * (dx * dx).sum(1)).sum()
            t = cy - s * R @ cx
            res = s * (x[b] - cx) @ R.T - (y[b] - cy)
        else:
            res = x[b] - y[b]
        dist = np.sqrt((res * res).sum(1))
        out["per_point"][b], out["err"][b] = dist, (wb * dist).sum() / tot
        out["transform"][b] = np.concatenate([[s], R.ravel(), t])
    return out


def oracle_horn_err(pred, gt, w=None, scale: bool = True) -> np.ndarray:
    """Errors ``[B]`` of the rigid / similarity alignment by Horn's closed form: the unit quaternion of the largest eigenvalue of
    the symmetric 4x4 matrix of the covariance (``numpy.linalg.eigh``), the eigenvalue over the variance as the scale."""
    x, y = np.asarray(pred, dtype=np.float64), np.asarray(gt, dtype=np.float64)
    B, N, _ = x.shape
    W = _frame_weights(w, B, N)
    err = np.zeros(B)
    for b in range(B):
        wb = W[b]
        tot = wb.sum()
        if tot == 0:
            continue
        cx, cy = (wb[:, None] * x[b]).sum(0) / tot, (wb[:, None] * y[b]).sum(0) / tot
        s, R = 1.0, np.eye(3)
        if _coincide(x[b], wb):
            cx = x[b][wb > 0][0]
        else:
            dx, dy = x[b] - cx, y[b] - cy
            S = (wb[:, None] * dx).T @ dy                      # S[a][b] = sum w dx_a dy_b
            Nm = np.array([
                [S[0, 0] + S[1, 1] + S[2, 2], S[1, 2] - S[2, 1], S[2, 0] - S[0, 2], S[0, 1] - S[1, 0]],
                [S[1, 2] - S[2, 1], S[0, 0] - S[1, 1] - S[2, 2], S[0, 1] + S[1, 0], S[2, 0] + S[0, 2]],
                [S[2, 0] - S[0, 2], S[0, 1] + S[1, 0], -S[0, 0] + S[1, 1] - S[2, 2], S[1, 2] + S[2, 1]],
                [S[0, 1] - S[1, 0], S[2, 0] + S[0, 2], S[1, 2] + S[2, 1], -S[0, 0] - S[1, 1] + S[2, 2]]])
            lam, vec = np.linalg.eigh(Nm)
            qw, qx, qy, qz = vec[:, -1]
            R = np.array([[qw * qw + qx * qx - qy * qy - qz * qz, 2 * (qx * qy - qw * qz), 2 * (qx * qz + qw * qy)],
                          [2 * (qx * qy + qw * qz), qw * qw - qx * qx + qy * qy - qz * qz, 2 * (qy * qz - qw * qx)],
                          [2 * (qx * qz - qw * qy), 2 * (qy * qz + qw * qx), qw * qw - qx * qx - qy * qy + qz * qz]])
            if scale:
                s = lam[-1] / (wb * (dx * dx).sum(1)).sum()
        res = s * (x[b] - cx) @ R.T - (y[b] - cy)
        err[b] = (wb * np.sqrt((res * res).sum(1))).sum() / tot
    return err


def parity_cases():
    """Every ``(name, pred, gt, w)`` the GPU parity test runs: the point counts across the frames-per-workgroup boundary and both
    regimes, with each weight variant; the frame counts at one small and one large point count; two mesh-sized frames; and the
    family offset by 1000 m."""
    cases = []
    for N in POINT_COUNTS:
        for kind in WEIGHT_KINDS:
            cases.append((f"N{N}-B3-{kind}", *make_case(11, 3, N, kind)))
    for B in FRAME_COUNTS:
        for N, kind in ((22, "frame"), (300, "shared")):
            cases.append((f"frames-N{N}-B{B}-{kind}", *make_case(12, B, N, kind)))
    cases.append((f"N{MESH_POINTS}-B{MESH_FRAMES}-none", *make_case(13, MESH_FRAMES, MESH_POINTS, "none")))
    cases.append((f"N{MESH_POINTS}-B{MESH_FRAMES}-frame", *make_case(13, MESH_FRAMES, MESH_POINTS, "frame")))
    for N, kind in ((22, "none"), (257, "frame")):
        cases.append((f"N{N}-B3-{kind}-offset1000", *make_case(14, 3, N, kind, offset=1000.0)))
    assert len({name for name, *_ in cases}) == len(cases)         # the names key the GPU test's cases: none may hide another
    return cases


def mirrored_case(seed: int = 21, B: int = 3, N: int = 22):
    """``gt`` is the mirror image (x -> -x) of ``pred``, rotated and moved: no proper rotation aligns them."""
    rng = np.random.default_rng(seed)
    pred = rng.uniform(-1.0, 1.0, (B, N, 3)) * np.array([1.6, 0.9, 0.5])
    gt = np.stack([(pred[b] * np.array([-1.0, 1.0, 1.0])) @ random_rotation(rng).T + rng.uniform(-0.4, 0.4, 3) for b in range(B)])
    return pred.astype(np.float32), gt.astype(np.float32)


def known_transform_case(seed: int = 22, B: int = 4, N: int = 30, scale: bool = True):
    """``gt = s R pred + t`` in float64, rounded to float32: ``(pred, gt, s [B], R [B][3][3], t [B][3])``."""
    rng = np.random.default_rng(seed)
    pred = (rng.uniform(-1.0, 1.0, (B, N, 3)) * np.array([1.6, 0.9, 0.5])).astype(np.float32)
    s = rng.uniform(0.6, 1.5, B) if scale else np.ones(B)
    R = np.stack([random_rotation(rng) for _ in range(B)])
    t = rng.uniform(-0.5, 0.5, (B, 3))
    gt = s[:, None, None] * np.einsum("bij,bnj->bni", R, pred.astype(np.float64)) + t[:, None, :]
    return pred, gt.astype(np.float32), s, R, t
