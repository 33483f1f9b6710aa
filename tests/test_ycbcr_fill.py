"""fsr1_ycbcr_fill / fsr1_rgb2ycbcr_fill (host, no GPU): the 8-bit fillers bit for bit at bits = 8, and at 10 bits the standards' codes for
black, white and the primaries — formed in exact rational arithmetic, as in test_rgb2ycbcr.py."""
import ctypes
from fractions import Fraction as Fr

import numpy as np
import pytest

from test_ycbcr import COLOURS

KR_KB = {"bt601": ("0.299", "0.114"), "bt709": ("0.2126", "0.0722"), "bt2020": ("0.2627", "0.0593")}


@pytest.mark.parametrize("full", [0, 1], ids=["limited", "full"])
@pytest.mark.parametrize("std", ["bt601", "bt709"])
def test_eight_bits_equal_the_existing_fillers(fsr, std, full):
    lib, standard = fsr.load(), {"bt601": fsr.YCBCR_BT601, "bt709": fsr.YCBCR_BT709}[std]
    for struct, stem in ((fsr.fsr1_ycbcr, "fsr1_ycbcr"), (fsr.fsr1_rgb2ycbcr, "fsr1_rgb2ycbcr")):
        old, new = struct(), struct()
        assert getattr(lib, "%s_%s" % (stem, std))(ctypes.byref(old), full) == 0 and getattr(lib, stem + "_fill")(ctypes.byref(new), standard, full, 8) == 0
        assert bytes(old) == bytes(new), (stem, std, full)


@pytest.mark.parametrize("std", ["bt2020", "bt709"])
def test_ten_bit_limited_codes_of_the_standard(fsr, std):
    conv, yc = getattr(fsr.RgbToYCbCr, std)(bits=10), getattr(fsr.YCbCr, std)(bits=10)
    kr, kb = (Fr(k) for k in KR_KB[std])
    for name, (r, g, b) in COLOURS.items():
        ey = kr * r + (1 - kr - kb) * g + kb * b
        exact = (64 + 876 * ey, 512 + 896 * (b - ey) / (2 * (1 - kb)), 512 + 896 * (r - ey) / (2 * (1 - kr)))
        want = [int(min(max(v, 0), 1023) + Fr(1, 2)) for v in exact]  # clamp, add a half, truncate
        p, got = np.array((r, g, b), np.float32), []
        for k in range(3):  # the pinned three-step form in binary32, then the code rule
            v = conv.bias[k] + conv.m[k, 0] * p[0]
            v = v + conv.m[k, 1] * p[1]
            v = v + conv.m[k, 2] * p[2]
            got.append(int(np.float32(min(max(v, np.float32(0)), np.float32(1023))) + np.float32(0.5)))
        assert got == want, (std, name, got, want)
        assert np.abs(yc.m.astype(np.float64) @ [float(v) for v in exact] + yc.bias - (r, g, b)).max() < 2e-6, (std, name)
    # the codes the standards print for 10 bits: black (64, 512, 512), white (940, 512, 512); BT.2020 red has Cr at its peak 960
    assert np.abs(yc.m.astype(np.float64) @ [940, 512, 512] + yc.bias - 1).max() < 2e-6 and np.abs(yc.m.astype(np.float64) @ [64, 512, 512] + yc.bias).max() < 2e-6


def test_nulls_and_unknown_arguments_are_refused(fsr):
    lib, y, r = fsr.load(), fsr.fsr1_ycbcr(), fsr.fsr1_rgb2ycbcr()
    for fill, s in ((lib.fsr1_ycbcr_fill, y), (lib.fsr1_rgb2ycbcr_fill, r)):
        assert fill(None, 0, 0, 8) == -1 and fill(ctypes.byref(s), 3, 0, 8) == -1 and fill(ctypes.byref(s), -1, 0, 8) == -1
        assert fill(ctypes.byref(s), 2, 0, 9) == -1 and fill(ctypes.byref(s), 2, 0, 0) == -1 and fill(ctypes.byref(s), 2, 1, 12) == 0
    with pytest.raises(fsr.Fsr1Error):
        fsr.YCbCr.bt2020(bits=9)
