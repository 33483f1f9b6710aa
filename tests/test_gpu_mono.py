"""Single-channel images (FORMAT_R16F / R32F / R8_UNORM: a (H,W), (N,H,W) or (N,1,H,W) tensor behind fsr.Mono) through EASU and RCAS.
The output for a luma image L is channel R of FsrEasuF / FsrRcasF on (L, L, L, 1): EXACT is bit-identical to channel 0 of the
CPU-evaluated reference rounded to the element type (uint8: every code); the default arithmetic is in the F class of the existing helpers
and bit-identical to channel R of the RGBA kernels on the replicated image with alpha 1 / 255.  RCAS is judged on the GPU's own
intermediary.  binary32 sources carry full 24-bit mantissas: the reference's luma*2 of (L, L, L) is 0.5 L + round(1.5 L), not 2 L."""
import ctypes
import importlib

import numpy as np
import pytest

from test_gpu_parity import assert_exact16, assert_exact32, assert_f_class
from test_gpu_planar import REFUSED
from test_gpu_rgb import same_bits
from test_gpu_unorm import check_codes, decode, encode, rgba8_frame

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
frames = importlib.import_module("fidelityfx-fsr_amd.frames")

# torch type, numpy type, EXACT comparison, columns one RCAS workgroup covers (two waves of 64 lanes x the columns a lane owns)
DTYPES = {"f16": (torch.float16, np.float16, assert_exact16, 2 * 64 * 4), "f32": (torch.float32, np.float32, assert_exact32, 2 * 64 * 2),
          "u8": (torch.uint8, np.uint8, None, 2 * 64 * 4)}
# smaller than a tile and than a lane's group | generic ratio, ragged, crosses the 64 x 16 EASU tiles | exact 2x: the shifted quads, the
# tile seam at column 64, an even width that is no multiple of 64 | (per dtype) RCAS strips: three columns more than a workgroup's, so
# a wave seam, a workgroup seam and a width that is no multiple of the group
SHAPES = [(5, 3, 17, 9), (97, 61, 131, 83), (66, 19, 132, 38), "rcas_seams"]


def plane(tdt, w, h, padded, n=1):
    """An empty (n,h,w) single-channel tensor: tight rows (element-wise kernels on odd widths) or rows padded to 16 bytes (wide ones)."""
    per16 = 16 // torch.zeros(0, dtype=tdt).element_size()
    return torch.zeros(n, h, (w + per16 - 1) // per16 * per16 if padded else w, dtype=tdt, device="cuda")[..., :w]


def source(dt, w, h, k):
    """Host luma frame in the element type: one channel of the synthetic frame (binary32: full mantissas; uint8: codes)."""
    if dt == "u8":
        return np.ascontiguousarray(rgba8_frame(w, h, k)[..., 1])
    l = frames.synthetic_frame(w, h, k=k, dtype=np.float32)[..., 1]
    return np.ascontiguousarray(l * np.float32(1.2345678) if dt == "f32" else l.astype(np.float16))


def rgba(dt, l):
    """(L, L, L, 1 | 255) in the element type."""
    return np.ascontiguousarray(np.stack([l, l, l, np.full_like(l, 255 if dt == "u8" else 1)], -1))


def as_f32(dt, x):
    return decode(x, 255) if dt == "u8" else x.astype(np.float32)


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def check(dt, got, want_f32, exact, what):
    """got (h,w) in the element type against channel 0 of the binary32 reference (h,w,4)."""
    if dt == "u8":
        check_codes(got, encode(want_f32[..., 0], 255), exact, what)
    elif exact:
        DTYPES[dt][2](got, want_f32[..., 0], what)
    else:
        assert_f_class(got, want_f32[..., 0], what)


EASU_WANT = {}  # (dt, shape) -> the CPU-evaluated EASU of the replicated source: shared by the layouts and arithmetics


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: s if isinstance(s, str) else "%dx%d_to_%dx%d" % s)
@pytest.mark.parametrize("padded", [False, True], ids=["tight", "padded"])
@pytest.mark.parametrize("exact", [True, False], ids=["exact", "default"])
@pytest.mark.parametrize("dt", sorted(DTYPES))
def test_mono_stages(fsr, port, dt, exact, padded, shape):
    tdt = DTYPES[dt][0]
    iw, ih, ow, oh = ((DTYPES[dt][3] + 3 + 3) // 4, 9, DTYPES[dt][3] + 3, 17) if shape == "rcas_seams" else shape
    math = fsr.FLAG_MATH_EXACT if exact else 0
    lum = source(dt, iw, ih, 5)
    con, rcon = port.FsrEasuCon(iw, ih, iw, ih, ow, oh), port.FsrRcasCon(0.25)
    src, mid, out = plane(tdt, iw, ih, padded), plane(tdt, ow, oh, padded), plane(tdt, ow, oh, padded)
    src.copy_(torch.from_numpy(lum[None]))
    fsr.easu(fsr.Mono(src), fsr.Mono(mid), con=con, flags=math)
    fsr.rcas(fsr.Mono(mid), fsr.Mono(out), con=rcon, flags=math)
    got_mid = host(mid)[0]
    if (dt, shape) not in EASU_WANT:
        EASU_WANT[dt, shape] = port.easu_f(as_f32(dt, rgba(dt, lum)), ow, oh, con)
    check(dt, got_mid, EASU_WANT[dt, shape], exact, "easu mono " + dt)
    check(dt, host(out)[0], port.rcas_f(as_f32(dt, rgba(dt, got_mid)), rcon), exact, "rcas mono " + dt)
    if exact:
        if shape == SHAPES[1]:
            fsr.rcas(fsr.Mono(mid), fsr.Mono(out), con=rcon, flags=math | fsr.FLAG_RCAS_DENOISE)
            check(dt, host(out)[0], port.rcas_f(as_f32(dt, rgba(dt, got_mid)), rcon, 1), True, "rcas denoise mono " + dt)
        return
    # channel R of the RGBA kernels of the element type on the replicated image
    i_mid, i_out = (torch.zeros(oh, ow, 4, dtype=tdt, device="cuda") for _ in range(2))
    fsr.easu(torch.from_numpy(rgba(dt, lum)).cuda(), i_mid, con=con)
    fsr.rcas(torch.from_numpy(rgba(dt, got_mid)).cuda(), i_out, con=rcon)
    same_bits(got_mid, host(i_mid)[..., 0], "easu: mono != channel R of RGBA")
    same_bits(host(out)[0], host(i_out)[..., 0], "rcas: mono != channel R of RGBA")


def test_mono_hdr_square(fsr, port):
    """`c *= c` (EASU alone; RCAS after its resolve) under EXACT, binary32, the exact-2x shape."""
    iw, ih, ow, oh = SHAPES[2]
    lum = source("f32", iw, ih, 5)
    con, rcon = port.FsrEasuCon(iw, ih, iw, ih, ow, oh), port.FsrRcasCon(0.25)
    src, mid, out = plane(torch.float32, iw, ih, True), plane(torch.float32, ow, oh, True), plane(torch.float32, ow, oh, True)
    src.copy_(torch.from_numpy(lum[None]))
    fsr.easu(fsr.Mono(src), fsr.Mono(mid), con=con, flags=fsr.FLAG_MATH_EXACT | fsr.FLAG_HDR_SQUARE)
    want = port.easu_f(rgba("f32", lum), ow, oh, con)[..., 0]
    assert_exact32(host(mid)[0], want * want, "easu EXACT hdr mono")
    fsr.rcas(fsr.Mono(mid), fsr.Mono(out), con=rcon, flags=fsr.FLAG_MATH_EXACT | fsr.FLAG_HDR_SQUARE)
    want = port.rcas_f(rgba("f32", host(mid)[0]), rcon)[..., 0]
    assert_exact32(host(out)[0], want * want, "rcas EXACT hdr mono")


@pytest.mark.parametrize("dt", sorted(DTYPES))
def test_mono_batch(fsr, port, dt):
    """Three frames in padded tensors, EXACT: the two dispatches, FSR_Filter with fused = "auto" and the stream pipeline."""
    tdt, ndt = DTYPES[dt][:2]
    iw, ih, ow, oh, n = 37, 11, 74, 22, 3
    lum = np.stack([source(dt, iw, ih, k) for k in range(n)])
    con, rcon = port.FsrEasuCon(iw, ih, iw, ih, ow, oh), port.FsrRcasCon(0.25)
    src = plane(tdt, iw, ih, True, n)
    src.copy_(torch.from_numpy(lum))
    mid, out, flt, pip = (plane(tdt, ow, oh, True, n) for _ in range(4))
    fsr.easu(fsr.Mono(src), fsr.Mono(mid), con=con, flags=fsr.FLAG_MATH_EXACT)
    fsr.rcas(fsr.Mono(mid), fsr.Mono(out), con=rcon, flags=fsr.FLAG_MATH_EXACT)
    filt = fsr.FSR_Filter()
    filt.OnCreate(slowFallback=True, exact=True, fused="auto")
    filt.OnCreateWindowSizeDependentResources(fsr.Mono(src), fsr.Mono(flt.unsqueeze(1)), ow, oh)  # (N,1,H,W)
    filt.Upscale(ow, oh, fsr.State(iw, ih, bUseRcas=True, rcasAttenuation=0.25))
    filt.OnDestroy()
    pipe = fsr.Pipeline(2)
    pipe.upscale(fsr.Mono(src), fsr.Mono(pip), sharpness=0.25, fused=2, flags=fsr.FLAG_MATH_EXACT)
    pipe.synchronize()
    pipe.close()
    got = host(out)
    same_bits(host(flt), got, "FSR_Filter auto mono batch")
    same_bits(host(pip), got, "pipeline mono batch")
    for k in range(n):
        want_mid = port.easu_f(as_f32(dt, rgba(dt, lum[k])), ow, oh, con)[..., 0]  # stored: rounded to the element type
        want_mid = encode(want_mid, 255).astype(np.uint8) if dt == "u8" else want_mid.astype(ndt)
        check(dt, got[k], port.rcas_f(as_f32(dt, rgba(dt, want_mid)), rcon), True, "chain EXACT mono frame %d" % k)


REFUSED_MONO = dict(REFUSED, color_dispatch=lambda L, F, i, o, r, c, rc: L.fsr1_color_dispatch(o, o, ctypes.byref(F.fsr1_color_stages(F.COLOR_SRTM, 0, 0, 0, 0, 0, None)), 0, None))


@pytest.mark.parametrize("what", sorted(REFUSED_MONO) + ["mono_to_planar"])
def test_mono_refusals(fsr, what):
    lib, to_planar = fsr.load(), what == "mono_to_planar"  # (= REFUSED's "planar_to_interleaved" call with planes as the other image)
    other = fsr.Planar(torch.zeros(3, 16, 16, dtype=torch.float16, device="cuda")) if to_planar else torch.zeros(16, 16, 4, dtype=torch.float16, device="cuda")
    i, o, r = (ctypes.byref(fsr.image_of(t)) for t in (fsr.Mono(plane(torch.float16, 8, 8, False)), fsr.Mono(plane(torch.float16, 16, 16, False)), other))
    cons = (fsr.FsrEasuCon(8, 8, 8, 8, 16, 16), fsr.FsrRcasCon(0.25))
    call = REFUSED_MONO["planar_to_interleaved" if to_planar else what]
    assert call(lib, fsr, i, o, r, *(a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)) for a in cons)) == -2
    assert b"single-channel" in lib.fsr1_last_error(), lib.fsr1_last_error()


@pytest.mark.parametrize("t", [lambda: torch.zeros(2, 8, 8, dtype=torch.int32, device="cuda"), lambda: torch.zeros(2, 3, 8, 8, dtype=torch.float16, device="cuda"),
                               lambda: torch.zeros(8, 16, dtype=torch.float16, device="cuda")[:, ::2]], ids=["int32", "three_channels", "strided_x"])
def test_mono_validation(fsr, t):
    with pytest.raises(fsr.Fsr1Error):
        fsr.image_of(fsr.Mono(t()))
    assert fsr.image_of(torch.zeros(2, 8, 8, dtype=torch.int32, device="cuda")).format == fsr.FORMAT_R10G10B10A2_UNORM  # a bare int32 tensor stays packed words
