"""Planar 8-bit RGB images (FORMAT_RGB8_UNORM_PLANAR, a uint8 (N,3,H,W) tensor behind fsr.Planar) through EASU and RCAS.  EXACT
reproduces every code of the CPU-evaluated FsrEasuF / FsrRcasF between RGBA8_UNORM's conversions; the default arithmetic is in the F
class of tests/test_gpu_unorm.py and byte-identical to the RGBA8_UNORM kernels.  RCAS is judged on the GPU's own intermediary."""
import ctypes

import numpy as np
import pytest

from test_gpu_planar import REFUSED, SHAPES, to_hwc
from test_gpu_unorm import check_codes, decode, encode, rgba8_frame

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

LAYOUTS = ["tight", "padded", "padded_shifted"]  # rows of w bytes | of a multiple of 16 | the same, base pointer one byte in


def planes(w, h, layout, n=None):
    """An empty uint8 planar tensor of w x h images; "padded_shifted" is a view whose first column is sliced off."""
    lead, x0 = (3,) if n is None else (n, 3), int(layout == "padded_shifted")
    row = w if layout == "tight" else (w + x0 + 15) // 16 * 16
    return torch.zeros(*lead, h, row, dtype=torch.uint8, device="cuda")[..., x0:x0 + w]


def to_planes(codes, layout):  # (..., H, W, 3) host codes -> planar device tensor
    t = planes(codes.shape[-2], codes.shape[-3], layout, None if codes.ndim == 3 else codes.shape[0])
    t.copy_(torch.from_numpy(np.ascontiguousarray(np.moveaxis(codes, -1, -3))))
    return t


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d_to_%dx%d" % s)
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("exact", [True, False], ids=["exact", "default"])
def test_planar_u8_stages(fsr, port, exact, layout, shape):
    (iw, ih, ow, oh), math = shape, fsr.FLAG_MATH_EXACT if exact else 0
    codes = rgba8_frame(iw, ih, 5)
    codes[..., 3] = 255
    con, rcon = port.FsrEasuCon(iw, ih, iw, ih, ow, oh), port.FsrRcasCon(0.25)
    src, mid, out = to_planes(codes[..., :3], layout), planes(ow, oh, layout), planes(ow, oh, layout)
    fsr.easu(fsr.Planar(src), fsr.Planar(mid), con=con, flags=math)
    fsr.rcas(fsr.Planar(mid), fsr.Planar(out), con=rcon, flags=math)
    got_mid = np.ascontiguousarray(np.concatenate([to_hwc(mid), np.full((oh, ow, 1), 255, np.uint8)], -1))  # alpha at its maximum
    want_mid = encode(port.easu_f(decode(codes, 255), ow, oh, con), 255)[..., :3]
    want_out = encode(port.rcas_f(decode(got_mid, 255), rcon), 255)[..., :3]
    check_codes(got_mid[..., :3], want_mid, exact, "easu planar u8")
    check_codes(to_hwc(out), want_out, exact, "rcas planar u8")
    if exact:
        if shape == SHAPES[1]:
            fsr.rcas(fsr.Planar(mid), fsr.Planar(out), con=rcon, flags=math | fsr.FLAG_RCAS_DENOISE)
            check_codes(to_hwc(out), encode(port.rcas_f(decode(got_mid, 255), rcon, 1), 255)[..., :3], True, "rcas denoise planar u8")
        return
    # the interleaved RGBA8_UNORM kernels on the same pixels with alpha 255
    i_mid, i_out = (torch.zeros(oh, ow, 4, dtype=torch.uint8, device="cuda") for _ in range(2))
    fsr.easu(torch.from_numpy(codes).cuda(), i_mid, con=con)
    fsr.rcas(torch.from_numpy(got_mid).cuda(), i_out, con=rcon)
    assert np.array_equal(got_mid, i_mid.cpu().numpy()), "easu: planar u8 != RGBA8"
    assert np.array_equal(to_hwc(out), i_out.cpu().numpy()[..., :3]), "rcas: planar u8 != RGBA8"


def test_planar_u8_batch(fsr, port):
    """Three frames in padded tensors, EXACT: the two dispatches, FSR_Filter with fused = "auto" and the stream pipeline."""
    iw, ih, ow, oh, n = 37, 11, 74, 22, 3
    codes = np.stack([rgba8_frame(iw, ih, k) for k in range(n)])
    con, rcon = port.FsrEasuCon(iw, ih, iw, ih, ow, oh), port.FsrRcasCon(0.25)
    src, (mid, out, flt, pip) = to_planes(codes[..., :3], "padded"), (planes(ow, oh, "padded", n) for _ in range(4))
    fsr.easu(fsr.Planar(src), fsr.Planar(mid), con=con, flags=fsr.FLAG_MATH_EXACT)
    fsr.rcas(fsr.Planar(mid), fsr.Planar(out), con=rcon, flags=fsr.FLAG_MATH_EXACT)
    filt = fsr.FSR_Filter()
    filt.OnCreate(slowFallback=True, exact=True, fused="auto")
    filt.OnCreateWindowSizeDependentResources(fsr.Planar(src), fsr.Planar(flt), ow, oh)
    filt.Upscale(ow, oh, fsr.State(iw, ih, bUseRcas=True, rcasAttenuation=0.25))
    filt.OnDestroy()
    pipe = fsr.Pipeline(2)
    pipe.upscale(fsr.Planar(src), fsr.Planar(pip), sharpness=0.25, fused=2, flags=fsr.FLAG_MATH_EXACT)
    pipe.synchronize()
    pipe.close()
    got = to_hwc(out)
    assert np.array_equal(to_hwc(flt), got) and np.array_equal(to_hwc(pip), got), "FSR_Filter auto / pipeline != two dispatches"
    for k in range(n):
        want_mid = encode(port.easu_f(decode(codes[k], 255), ow, oh, con), 255)  # stored: the 8-bit intermediary
        want_mid[..., 3] = 255
        check_codes(got[k], encode(port.rcas_f(decode(want_mid, 255), rcon), 255)[..., :3], True, "chain EXACT planar u8 frame %d" % k)


def test_planar_u8_strict_is_exact(fsr):
    iw, ih, ow, oh = SHAPES[2]
    src = to_planes(rgba8_frame(iw, ih, 5)[..., :3], "padded")
    e_mid, e_out, s_mid, s_out = (planes(ow, oh, "padded") for _ in range(4))
    for math, mid, out in ((fsr.FLAG_MATH_EXACT, e_mid, e_out), (fsr.FLAG_MATH_STRICT, s_mid, s_out)):
        fsr.easu(fsr.Planar(src), fsr.Planar(mid), flags=math)
        fsr.rcas(fsr.Planar(mid), fsr.Planar(out), flags=math)
    assert np.array_equal(to_hwc(s_mid), to_hwc(e_mid)) and np.array_equal(to_hwc(s_out), to_hwc(e_out)), "STRICT != EXACT on planar u8"


@pytest.mark.parametrize("what", sorted(REFUSED) + ["u8_to_f16_planes"])
def test_planar_u8_refusals(fsr, what):
    lib, u8_f16 = fsr.load(), what == "u8_to_f16_planes"  # (= the planar -> interleaved call with fp16 planes as the other image)
    r = fsr.Planar(torch.zeros(3, 16, 16, dtype=torch.float16, device="cuda")) if u8_f16 else torch.zeros(16, 16, 4, dtype=torch.uint8, device="cuda")
    i, o, r = (ctypes.byref(fsr.image_of(t)) for t in (fsr.Planar(planes(8, 8, "tight")), fsr.Planar(planes(16, 16, "tight")), r))
    cons = (fsr.FsrEasuCon(8, 8, 8, 8, 16, 16), fsr.FsrRcasCon(0.25))
    assert REFUSED["planar_to_interleaved" if u8_f16 else what](lib, fsr, i, o, r, *(a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)) for a in cons)) == -2
    assert b"planar" in lib.fsr1_last_error(), lib.fsr1_last_error()
