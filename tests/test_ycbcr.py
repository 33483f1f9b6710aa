"""fsr1_ycbcr_bt601 / fsr1_ycbcr_bt709 (host, no GPU): raw 8-bit codes in, RGB in {0 to 1} out, on triples whose answer the standards give."""
import numpy as np
import pytest

KR_KB = {"bt601": (0.299, 0.114), "bt709": (0.2126, 0.0722)}
COLOURS = {"black": (0, 0, 0), "white": (1, 1, 1), "red": (1, 0, 0), "green": (0, 1, 0), "blue": (0, 0, 1)}


@pytest.mark.parametrize("full", [False, True], ids=["limited", "full"])
@pytest.mark.parametrize("std", sorted(KR_KB))
def test_matrix_helpers_on_known_triples(fsr, std, full):
    yc = getattr(fsr.YCbCr, std)(full_range=full)
    assert yc.siting == fsr.CHROMA_LEFT and yc.m.dtype == np.float32
    (kr, kb), (y0, ys, cs) = KR_KB[std], (0, 255, 255) if full else (16, 219, 224)
    for name, rgb in COLOURS.items():
        ey = kr * rgb[0] + (1 - kr - kb) * rgb[1] + kb * rgb[2]  # the forward transform of the standard, unquantised codes
        codes = np.array([y0 + ys * ey, 128 + cs * (rgb[2] - ey) / (2 * (1 - kb)), 128 + cs * (rgb[0] - ey) / (2 * (1 - kr))])
        got = yc.m.astype(np.float64) @ codes + yc.bias
        assert np.abs(got - rgb).max() < 2e-6, (std, full, name, got)
    # the codes the standards print: limited-range black and white are (16, 128, 128) and (235, 128, 128), BT.601 red is (81, 90, 240)
    if not full:
        assert np.abs(yc.m.astype(np.float64) @ [235, 128, 128] + yc.bias - 1).max() < 2e-6
        if std == "bt601":
            assert np.abs(yc.m.astype(np.float64) @ [81, 90, 240] + yc.bias - [1, 0, 0]).max() < 0.004  # (integer codes: within a code)


def test_null_is_refused(fsr):
    assert fsr.load().fsr1_ycbcr_bt601(None, 0) == -1 and fsr.load().fsr1_ycbcr_bt709(None, 1) == -1
