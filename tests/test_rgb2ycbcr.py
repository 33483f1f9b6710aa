"""fsr1_rgb2ycbcr_bt601 / fsr1_rgb2ycbcr_bt709 (host, no GPU): the eight corners of the RGB cube through the numpy restatement of the NV12
store's conversion (test_gpu_nv12_out.reference_nv12) give exactly the codes the standards' Kr / Kb give.  Those are formed in exact
rational arithmetic, not in double: full-range yellow has Cb = 1/2 exactly (and blue Cb, red Cr = 255 1/2), where a double evaluation
lands a hair to either side of the tie and the code round-half-up defines (1) would depend on the order of its operations."""
import itertools
from fractions import Fraction as Fr

import numpy as np
import pytest

from test_gpu_nv12_out import reference_nv12
from test_ycbcr import KR_KB

CORNERS = list(itertools.product((0, 1), repeat=3))


def code(v):
    return int(min(max(v, 0), 255) + Fr(1, 2))  # clamp, add a half, truncate


@pytest.mark.parametrize("full", [False, True], ids=["limited", "full"])
@pytest.mark.parametrize("std", sorted(KR_KB))
def test_cube_corners_give_the_standards_codes(fsr, std, full):
    conv = getattr(fsr.RgbToYCbCr, std)(full_range=full)
    assert conv.siting == fsr.CHROMA_CENTER and conv.m.dtype == np.float32
    (kr, kb), (y0, ys, cs) = (Fr(str(k)) for k in KR_KB[std]), (0, 255, 255) if full else (16, 219, 224)
    want = {}
    for r, g, b in CORNERS:
        ey = kr * r + (1 - kr - kb) * g + kb * b
        want[r, g, b] = (code(y0 + ys * ey), code(128 + cs * (b - ey) / (2 * (1 - kb))), code(128 + cs * (r - ey) / (2 * (1 - kr))))
        y, c = reference_nv12(np.full((2, 2, 3), (r, g, b), np.float32), conv)  # a 2 x 2 image of one colour: four Y codes, one pair
        assert (y == want[r, g, b][0]).all() and tuple(c[0, 0]) == want[r, g, b][1:], (std, full, (r, g, b), y, c, want[r, g, b])
    assert want[1, 1, 1] == ((255, 128, 128) if full else (235, 128, 128)) and want[0, 0, 0] == ((0, 128, 128) if full else (16, 128, 128))


def test_null_is_refused(fsr):
    assert fsr.load().fsr1_rgb2ycbcr_bt601(None, 0) == -1 and fsr.load().fsr1_rgb2ycbcr_bt709(None, 1) == -1
