"""Packed 3-channel RGB images (FORMAT_RGB16F / RGB32F / RGB8_UNORM: a (N,H,W,3) or channels_last tensor behind fsr.Rgb) through EASU
and RCAS.  EXACT is bit-identical to the CPU-evaluated FsrEasuF / FsrRcasF rounded to the element type (uint8: every code, between
RGBA8_UNORM's conversions); the default arithmetic is in the F class of the existing helpers and bit-identical to the RGBA kernels on
the same pixels with alpha 1 / 255.  RCAS is judged on the GPU's own intermediary."""
import ctypes
import importlib

import numpy as np
import pytest

from test_gpu_parity import assert_exact16, assert_exact32, assert_f_class
from test_gpu_planar import REFUSED, SHAPES
from test_gpu_unorm import check_codes, decode, encode, rgba8_frame

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
frames = importlib.import_module("fidelityfx-fsr_amd.frames")

DTYPES = {"f16": (torch.float16, np.float16, assert_exact16), "f32": (torch.float32, np.float32, assert_exact32), "u8": (torch.uint8, np.uint8, None)}
# rows of 3 w elements | of a multiple of 16 bytes | the same, base pointer one pixel in | a (N,3,H,W) tensor in channels_last
LAYOUTS = ["tight", "padded", "padded_shifted", "channels_last"]


def image(tdt, w, h, layout, n=1):
    """An empty w x h 3-channel image: (what goes into fsr.Rgb, its (n,h,w,3) view)."""
    if layout == "channels_last":
        t = torch.zeros(n, 3, h, w, dtype=tdt, device="cuda").contiguous(memory_format=torch.channels_last)
        return t, t.permute(0, 2, 3, 1)
    x0 = 3 * int(layout == "padded_shifted")
    per16 = 16 // torch.zeros(0, dtype=tdt).element_size()
    row = 3 * w if layout == "tight" else (3 * w + x0 + per16 - 1) // per16 * per16
    v = torch.zeros(n, h, row, dtype=tdt, device="cuda")[..., x0:x0 + 3 * w].unflatten(-1, (w, 3))
    return v, v


def host(view, alpha=None):
    """(n,h,w,3) device view -> host array of frame 0 (or all frames), optionally with an alpha channel of `alpha`."""
    torch.cuda.synchronize()
    a = view.cpu().numpy()
    return np.ascontiguousarray(a if alpha is None else np.concatenate([a, np.full_like(a[..., :1], alpha)], -1))


def source(dt, w, h, k):  # RGBA host frame in the element type, alpha at its maximum
    if dt == "u8":
        f = rgba8_frame(w, h, k)
        f[..., 3] = 255
        return f
    return frames.synthetic_frame(w, h, k=k, dtype=DTYPES[dt][1])


EASU_WANT = {}  # (dt, shape) -> the CPU-evaluated EASU of source(dt, ..., 5): shared by the layouts and arithmetics


def as_f32(dt, x):
    return decode(x, 255) if dt == "u8" else x.astype(np.float32)


def check(dt, got, want_f32, exact, what):
    """got (.., 3) in the element type against the binary32 reference (.., 4)."""
    if dt == "u8":
        check_codes(got, encode(want_f32, 255)[..., :3], exact, what)
    elif exact:
        DTYPES[dt][2](got, want_f32[..., :3], what)
    else:
        assert_f_class(got, want_f32[..., :3], what)


def same_bits(a, b, what):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8)), what


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d_to_%dx%d" % s)
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("exact", [True, False], ids=["exact", "default"])
@pytest.mark.parametrize("dt", sorted(DTYPES))
def test_rgb_stages(fsr, port, dt, exact, layout, shape):
    tdt, one = DTYPES[dt][0], 255 if dt == "u8" else 1
    (iw, ih, ow, oh), math = shape, fsr.FLAG_MATH_EXACT if exact else 0
    rgba = source(dt, iw, ih, 5)
    con, rcon = port.FsrEasuCon(iw, ih, iw, ih, ow, oh), port.FsrRcasCon(0.25)
    (src, src_v), (mid, mid_v), (out, out_v) = image(tdt, iw, ih, layout), image(tdt, ow, oh, layout), image(tdt, ow, oh, layout)
    src_v.copy_(torch.from_numpy(rgba[None, ..., :3]))
    fsr.easu(fsr.Rgb(src), fsr.Rgb(mid), con=con, flags=math)
    fsr.rcas(fsr.Rgb(mid), fsr.Rgb(out), con=rcon, flags=math)
    got_mid = host(mid_v, one)[0]
    if (dt, shape) not in EASU_WANT:
        EASU_WANT[dt, shape] = port.easu_f(as_f32(dt, rgba), ow, oh, con)
    check(dt, got_mid[..., :3], EASU_WANT[dt, shape], exact, "easu rgb " + dt)
    check(dt, host(out_v)[0], port.rcas_f(as_f32(dt, got_mid), rcon), exact, "rcas rgb " + dt)
    if exact:
        if shape == SHAPES[1]:
            fsr.rcas(fsr.Rgb(mid), fsr.Rgb(out), con=rcon, flags=math | fsr.FLAG_RCAS_DENOISE)
            check(dt, host(out_v)[0], port.rcas_f(as_f32(dt, got_mid), rcon, 1), True, "rcas denoise rgb " + dt)
        return
    # the RGBA kernels of the element type on the same pixels with alpha 1 / 255
    i_mid, i_out = (torch.zeros(oh, ow, 4, dtype=tdt, device="cuda") for _ in range(2))
    fsr.easu(torch.from_numpy(rgba).cuda(), i_mid, con=con)
    fsr.rcas(torch.from_numpy(got_mid).cuda(), i_out, con=rcon)
    torch.cuda.synchronize()
    same_bits(got_mid, i_mid.cpu().numpy(), "easu: rgb != RGBA")
    same_bits(host(out_v)[0], i_out.cpu().numpy()[..., :3], "rcas: rgb != RGBA")


@pytest.mark.parametrize("dt", sorted(DTYPES))
def test_rgb_batch(fsr, port, dt):
    """Three frames in padded tensors, EXACT: the two dispatches, FSR_Filter with fused = "auto" and the stream pipeline."""
    tdt, one = DTYPES[dt][0], 255 if dt == "u8" else 1
    iw, ih, ow, oh, n = 37, 11, 74, 22, 3
    rgba = np.stack([source(dt, iw, ih, k) for k in range(n)])
    con, rcon = port.FsrEasuCon(iw, ih, iw, ih, ow, oh), port.FsrRcasCon(0.25)
    src = image(tdt, iw, ih, "padded", n)[1]
    src.copy_(torch.from_numpy(rgba[..., :3]))
    mid, out, flt, pip = (image(tdt, ow, oh, "padded", n)[1] for _ in range(4))
    fsr.easu(fsr.Rgb(src), fsr.Rgb(mid), con=con, flags=fsr.FLAG_MATH_EXACT)
    fsr.rcas(fsr.Rgb(mid), fsr.Rgb(out), con=rcon, flags=fsr.FLAG_MATH_EXACT)
    filt = fsr.FSR_Filter()
    filt.OnCreate(slowFallback=True, exact=True, fused="auto")
    filt.OnCreateWindowSizeDependentResources(fsr.Rgb(src), fsr.Rgb(flt), ow, oh)
    filt.Upscale(ow, oh, fsr.State(iw, ih, bUseRcas=True, rcasAttenuation=0.25))
    filt.OnDestroy()
    pipe = fsr.Pipeline(2)
    pipe.upscale(fsr.Rgb(src), fsr.Rgb(pip), sharpness=0.25, fused=2, flags=fsr.FLAG_MATH_EXACT)
    pipe.synchronize()
    pipe.close()
    got = host(out)
    same_bits(host(flt), got, "FSR_Filter auto rgb batch")
    same_bits(host(pip), got, "pipeline rgb batch")
    for k in range(n):
        want_mid = port.easu_f(as_f32(dt, rgba[k]), ow, oh, con)  # stored: rounded to the element type
        want_mid = encode(want_mid, 255).astype(np.uint8) if dt == "u8" else want_mid.astype(DTYPES[dt][1])
        want_mid[..., 3] = one
        check(dt, got[k], port.rcas_f(as_f32(dt, want_mid), rcon), True, "chain EXACT rgb frame %d" % k)


def test_rgb_strict_is_exact(fsr):
    iw, ih, ow, oh = SHAPES[2]
    src = image(torch.uint8, iw, ih, "padded")[1]
    src.copy_(torch.from_numpy(rgba8_frame(iw, ih, 5)[None, ..., :3]))
    e_mid, e_out, s_mid, s_out = (image(torch.uint8, ow, oh, "padded")[1] for _ in range(4))
    for math, mid, out in ((fsr.FLAG_MATH_EXACT, e_mid, e_out), (fsr.FLAG_MATH_STRICT, s_mid, s_out)):
        fsr.easu(fsr.Rgb(src), fsr.Rgb(mid), flags=math)
        fsr.rcas(fsr.Rgb(mid), fsr.Rgb(out), flags=math)
    assert np.array_equal(host(s_mid), host(e_mid)) and np.array_equal(host(s_out), host(e_out)), "STRICT != EXACT on rgb u8"


REFUSED_RGB = dict(REFUSED, color_dispatch=lambda L, F, i, o, r, c, rc: L.fsr1_color_dispatch(o, o, ctypes.byref(F.fsr1_color_stages(F.COLOR_SRTM, 0, 0, 0, 0, 0, None)), 0, None))


@pytest.mark.parametrize("what", sorted(REFUSED_RGB) + ["rgb_to_planar"])
def test_rgb_refusals(fsr, what):
    lib, to_planar = fsr.load(), what == "rgb_to_planar"  # (= REFUSED's "planar_to_interleaved" call with planes as the other image)
    other = fsr.Planar(torch.zeros(3, 16, 16, dtype=torch.float16, device="cuda")) if to_planar else torch.zeros(16, 16, 4, dtype=torch.float16, device="cuda")
    i, o, r = (ctypes.byref(fsr.image_of(t)) for t in (fsr.Rgb(image(torch.float16, 8, 8, "tight")[0]), fsr.Rgb(image(torch.float16, 16, 16, "tight")[0]), other))
    cons = (fsr.FsrEasuCon(8, 8, 8, 8, 16, 16), fsr.FsrRcasCon(0.25))
    call = REFUSED_RGB["planar_to_interleaved" if to_planar else what]
    assert call(lib, fsr, i, o, r, *(a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)) for a in cons)) == -2
    assert b"3-channel" in lib.fsr1_last_error(), lib.fsr1_last_error()


@pytest.mark.parametrize("t", [lambda: torch.zeros(8, 8, 4, dtype=torch.float16, device="cuda")[..., :3], lambda: torch.zeros(8, 8, 3, dtype=torch.int32, device="cuda")],
                         ids=["pixel_stride_4", "int32"])
def test_rgb_validation(fsr, t):
    with pytest.raises(fsr.Fsr1Error):
        fsr.image_of(fsr.Rgb(t()))
