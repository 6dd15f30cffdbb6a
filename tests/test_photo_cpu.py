"""The L1/SSIM photometric kernels' resources, cross-compiled (no GPU needed)."""
import re
import shutil
import sys

import pytest

from conftest import REPO

# VGPR budget of the forward per (BORDER, GRAD) at C = 3, 2, 1: the figures of
# the two-kernel version this file replaced (measured with the same tool)
FWD_VGPR = {(1, 1): (125, 94, 66), (0, 1): (119, 82, 63), (1, 0): (85, 66, 53), (0, 0): (85, 66, 53)}
FWD_LDS = {3: 12288, 2: 8192, 1: 4096}


@pytest.mark.skipif(shutil.which("/opt/rocm/bin/hipcc") is None, reason="hipcc not available")
def test_photo_kernels_fit_their_register_budget():
    """photo.hip has one forward (12 instantiations: BORDER x GRAD x C in 1..3),
    one final and one backward kernel; none spills to scratch and none needs
    more registers or LDS than before the single-scale twins were folded in."""
    sys.path.insert(0, str(REPO / "tools"))
    import kernel_resources

    res = kernel_resources.resources(REPO / "unsamflow_amd" / "csrc" / "photo.hip")
    assert len(res) == 14, [r[0] for r in res]
    fwd = {}
    for name, vgpr, lds, scratch in res:
        assert scratch == 0, (name, scratch)
        m = re.match(r"photo_fwd_kernelILb(\d)ELb(\d)ELi(\d)E", name)
        if m:
            border, grad, C = (int(v) for v in m.groups())
            fwd[border, grad, C] = (vgpr, lds)
    assert sorted(fwd) == [(b, g, c) for b in (0, 1) for g in (0, 1) for c in (1, 2, 3)]
    for (border, grad, C), (vgpr, lds) in fwd.items():
        assert vgpr <= FWD_VGPR[border, grad][3 - C] and lds <= FWD_LDS[C], (border, grad, C, vgpr, lds)
    (final,) = [r for r in res if r[0].startswith("photo_final_kernel")]
    (bwd,) = [r for r in res if r[0].startswith("photo_bwd_kernel")]
    assert final[1] <= 36 and bwd[1] <= 24, (final, bwd)
