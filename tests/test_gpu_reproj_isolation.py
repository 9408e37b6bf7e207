"""A frame with a TARGETED joint of non-zero confidence at Z = 0 (the projected joint term divides by Z as it stands) is non-finite
in its own row, and every other frame of the call is what it is without that frame, bit for bit (``include/k2b.h``, Conventions;
DESIGN.md 4.4c and 4.4d).  Both fit kernels in every launch shape, 3 and 17 frames, the evaluate-only closure and an Adam fit.
A NaN is a value, not a fault: nothing here provokes one."""
import numpy as np
import pytest
import torch

from keypoints2body_amd import native
from tests import reproj_common as R

pytestmark = pytest.mark.gpu

ADAM_ITERS = 5


def _adam(case, shape, rows=None):
    cfg = R.fit_config(case, shape)
    cfg.num_iters, cfg.step_size = ADAM_ITERS, 1e-2
    out, _ = R.device_call(case, cfg, want_grad=True, rows=rows)
    return {k: v.cpu().numpy() for k, v in out.items()}


@pytest.mark.parametrize("frames,bad", [(3, 1), (17, 6), (17, 16)])
@pytest.mark.parametrize("kind", R.BOTH)
def test_a_targeted_joint_at_depth_zero_stays_in_its_own_frame(kind, frames, bad):
    root_z = R.native_root_z(kind)
    case = R.z0_case(kind, True, root_z, conf_root=1.0, frames=frames, bad=(bad,))
    benign = R.z0_case(kind, True, root_z, conf_root=0.0, frames=frames, bad=(bad,))       # the same inputs, the root's confidence zero
    others = [f for f in range(frames) if f != bad]
    for shape in R.shapes_of(kind):
        loss, grad = R.device_eval(case, shape, finite=False)
        assert not np.isfinite(loss[bad]), f"{case.name} shape {shape}: the frame's loss is {loss[bad]}"
        ref_loss, ref_grad = R.device_eval(benign, shape)
        assert np.isfinite(ref_loss).all() and np.isfinite(ref_grad).all()
        assert np.array_equal(loss[others], ref_loss[others]) and np.array_equal(grad[others], ref_grad[others]), (case.name, shape)
        alone_loss, alone_grad = R.device_eval(case, shape, rows=others)                  # the call without the frame
        assert np.array_equal(loss[others], alone_loss) and np.array_equal(grad[others], alone_grad), (case.name, shape)
        fit, fit_ref, fit_alone = _adam(case, shape), _adam(benign, shape), _adam(case, shape, rows=others)
        assert not np.isfinite(fit["loss"][bad])
        for k in native.PARAM_KEYS + ("loss", "grad"):
            assert np.isfinite(fit_ref[k]).all(), k
            assert np.array_equal(fit[k][others], fit_ref[k][others]), f"{case.name} shape {shape}: {k} of another frame moved"
            assert np.array_equal(fit[k][others], fit_alone[k]), f"{case.name} shape {shape}: {k} depends on the frame's presence"
    torch.cuda.synchronize()
