"""Planar RGB images (FORMAT_RGB16F_PLANAR / RGB32F_PLANAR, a (N,3,H,W) tensor behind fsr.Planar) through EASU and RCAS.
EXACT is bit-identical to the CPU-evaluated FsrEasuF / FsrRcasF; the default arithmetic is in the F class of tests/test_gpu_parity.py
and bit-identical to the interleaved kernels on the same pixels with alpha 1.  RCAS is judged on the GPU's own intermediary."""
import ctypes
import importlib

import numpy as np
import pytest

from test_gpu_parity import assert_exact16, assert_exact32, assert_f_class

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
frames = importlib.import_module("fidelityfx-fsr_amd.frames")

DTYPES = {"f16": (torch.float16, np.float16, assert_exact16), "f32": (torch.float32, np.float32, assert_exact32)}
# smaller than a tile and than a lane's four pixels | generic ratio, ragged, crosses the 64 x 16 EASU tiles | exact 2x (the shifted
# quads) | RCAS strips: the wave seam at column 256, the workgroup seam at 512, width mod 4 = 3
SHAPES = [(5, 3, 17, 9), (97, 61, 131, 83), (66, 19, 132, 38), (130, 9, 515, 17)]


def planes(tdt, w, h, padded, n=None):
    """An empty planar tensor of w x h images: tight rows (element-wise kernels on odd widths) or rows padded to 8 elements (wide ones)."""
    lead = (3,) if n is None else (n, 3)
    return torch.zeros(*lead, h, (w + 7) // 8 * 8 if padded else w, dtype=tdt, device="cuda")[..., :w]


def to_planes(rgb, tdt, padded):
    """(..., H, W, 3) host array -> planar device tensor."""
    t = planes(tdt, rgb.shape[-2], rgb.shape[-3], padded, None if rgb.ndim == 3 else rgb.shape[0])
    t.copy_(torch.from_numpy(np.ascontiguousarray(np.moveaxis(rgb, -1, -3))))
    return t


def to_hwc(t, alpha=False):
    """planar device tensor -> (..., H, W, 3 | 4) host array, alpha = 1."""
    torch.cuda.synchronize()
    a = np.moveaxis(t.cpu().numpy(), -3, -1)
    return np.ascontiguousarray(np.concatenate([a, np.ones_like(a[..., :1])], -1) if alpha else a)


def same_bits(a, b, what):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8)), what


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d_to_%dx%d" % s)
@pytest.mark.parametrize("padded", [False, True], ids=["tight", "padded"])
@pytest.mark.parametrize("exact", [True, False], ids=["exact", "default"])
@pytest.mark.parametrize("dt", sorted(DTYPES))
def test_planar_stages(fsr, port, dt, exact, padded, shape):
    tdt, ndt, assert_exact = DTYPES[dt]
    iw, ih, ow, oh = shape
    math = fsr.FLAG_MATH_EXACT if exact else 0
    rgba = frames.synthetic_frame(iw, ih, k=5, dtype=ndt)
    con, rcon = port.FsrEasuCon(iw, ih, iw, ih, ow, oh), port.FsrRcasCon(0.25)
    src, mid, out = to_planes(rgba[..., :3], tdt, padded), planes(tdt, ow, oh, padded), planes(tdt, ow, oh, padded)
    fsr.easu(fsr.Planar(src), fsr.Planar(mid), con=con, flags=math)
    fsr.rcas(fsr.Planar(mid), fsr.Planar(out), con=rcon, flags=math)
    got_mid = to_hwc(mid, alpha=True)
    want_mid = port.easu_f(rgba.astype(np.float32), ow, oh, con)[..., :3]
    want_out = port.rcas_f(got_mid.astype(np.float32), rcon)[..., :3]
    if exact:
        assert_exact(got_mid[..., :3], want_mid, "easu EXACT planar " + dt)
        assert_exact(to_hwc(out), want_out, "rcas EXACT planar " + dt)
        if shape == SHAPES[1]:
            fsr.rcas(fsr.Planar(mid), fsr.Planar(out), con=rcon, flags=math | fsr.FLAG_RCAS_DENOISE)
            assert_exact(to_hwc(out), port.rcas_f(got_mid.astype(np.float32), rcon, 1)[..., :3], "rcas EXACT denoise planar " + dt)
        return
    assert_f_class(got_mid[..., :3], want_mid, "easu F planar " + dt)
    assert_f_class(to_hwc(out), want_out, "rcas F planar " + dt)
    # the interleaved kernels on the same pixels with alpha 1
    i_mid, i_out = (torch.zeros(oh, ow, 4, dtype=tdt, device="cuda") for _ in range(2))
    fsr.easu(torch.from_numpy(rgba).cuda(), i_mid, con=con)
    fsr.rcas(torch.from_numpy(got_mid).cuda(), i_out, con=rcon)
    torch.cuda.synchronize()
    same_bits(got_mid, i_mid.cpu().numpy(), "easu F: planar != interleaved")
    same_bits(to_hwc(out), i_out.cpu().numpy()[..., :3], "rcas F: planar != interleaved")


@pytest.mark.parametrize("dt", sorted(DTYPES))
def test_planar_batch_with_padded_pitch(fsr, port, dt):
    """Three frames in padded tensors, EXACT: the two dispatches, FSR_Filter with fused = "auto" and the stream pipeline."""
    tdt, ndt, assert_exact = DTYPES[dt]
    iw, ih, ow, oh, n = 37, 11, 74, 22, 3
    rgba = np.stack([frames.synthetic_frame(iw, ih, k=k, dtype=ndt) for k in range(n)])
    con, rcon = port.FsrEasuCon(iw, ih, iw, ih, ow, oh), port.FsrRcasCon(0.25)
    src = to_planes(rgba[..., :3], tdt, True)
    mid, out, flt, pip = (planes(tdt, ow, oh, True, n) for _ in range(4))
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
    same_bits(to_hwc(flt), got, "FSR_Filter auto planar batch")
    same_bits(to_hwc(pip), got, "pipeline planar batch")
    for k in range(n):
        want_mid = port.easu_f(rgba[k].astype(np.float32), ow, oh, con).astype(ndt)  # stored: RTNE to the plane's type
        want_mid[..., 3] = 1
        assert_exact(got[k], port.rcas_f(want_mid.astype(np.float32), rcon)[..., :3], "chain EXACT planar frame %d" % k)


REFUSED = {
    "packed_fp16": lambda L, F, i, o, r, c, rc: L.fsr1_easu_dispatch(i, o, c, F.FLAG_MATH_PACKED_FP16, None),
    "colour_stages": lambda L, F, i, o, r, c, rc: L.fsr1_easu_dispatch_ex(i, o, c, 0, ctypes.byref(F.fsr1_color_stages(F.COLOR_SRTM, 0, 0, 0, 0, 0, None)), None),
    "easu_rcas_fused": lambda L, F, i, o, r, c, rc: L.fsr1_easu_rcas_fused_dispatch(i, o, c, rc, 0, None),
    "band": lambda L, F, i, o, r, c, rc: L.fsr1_easu_dispatch_band(i, o, c, 0, 0, 0, None),
    "passthrough_alpha": lambda L, F, i, o, r, c, rc: L.fsr1_rcas_dispatch(o, o, rc, F.FLAG_RCAS_PASSTHROUGH_ALPHA, None),
    "planar_to_interleaved": lambda L, F, i, o, r, c, rc: L.fsr1_easu_dispatch(i, r, c, 0, None),
}


@pytest.mark.parametrize("what", sorted(REFUSED))
def test_planar_refusals(fsr, what):
    lib = fsr.load()
    src, dst, rgba = planes(torch.float16, 8, 8, False), planes(torch.float16, 16, 16, False), torch.zeros(16, 16, 4, dtype=torch.float16, device="cuda")
    i, o, r = (ctypes.byref(fsr.image_of(t)) for t in (fsr.Planar(src), fsr.Planar(dst), rgba))
    con, rcon = fsr.FsrEasuCon(8, 8, 8, 8, 16, 16), fsr.FsrRcasCon(0.25)
    u32p = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32))  # noqa: E731
    assert REFUSED[what](lib, fsr, i, o, r, u32p(con), u32p(rcon)) == -2
    assert b"planar" in lib.fsr1_last_error(), lib.fsr1_last_error()


def test_planar_needs_adjacent_planes(fsr):
    with pytest.raises(fsr.Fsr1Error, match="plane stride"):
        fsr.image_of(fsr.Planar(torch.zeros(3, 9, 16, dtype=torch.float16, device="cuda")[:, :8]))
