"""NV12 frames (FORMAT_NV12 behind fsr.Nv12: an 8-bit Y plane and a half-resolution plane of Cb, Cr pairs) through the EASU that
converts while it stages, into planar RGB of any of the three plane types.  The reference is reference_rgb(): the conversion pinned in
include/fsr1_hip.h restated in numpy float32; EASU on it is the oracle's (EXACT: bit for bit) and the planar binary32 kernel's on the
GPU (both arithmetics: bit for bit — the records are the same, so a contracted multiply-add in the conversion shows here)."""
import ctypes
import functools
import importlib

import numpy as np
import pytest

from test_gpu_parity import assert_exact16, assert_exact32, assert_f_class
from test_gpu_planar import planes, same_bits, to_hwc, to_planes
from test_gpu_unorm import check_codes, decode, encode

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
frames = importlib.import_module("fidelityfx-fsr_amd.frames")

OUT = {"f16": (torch.float16, np.float16), "f32": (torch.float32, np.float32), "u8": (torch.uint8, np.uint8)}
# siting -> (fsr1_ycbcr.siting, the matrix it is tested with, full range)
SITINGS = {"replicate": (0, "bt601", False), "left": (1, "bt709", False), "center": (2, "bt601", True)}
# odd both ways, a 3 x 2 chroma plane, smaller than a tile: every chroma clamp | generic ratio, ragged, crosses tiles | exact 2x, odd
# height | minifying: the footprint of a tile is 154 luma texels and 80 chroma pairs wide, so the staging's 64-column walk takes a
# second and a third trip (the only shape that does)
SHAPES = [(5, 3, 17, 9), (97, 61, 131, 83), (66, 19, 132, 38), (150, 8, 64, 8)]


def ycbcr_of(fsr, siting):
    code, matrix, full = SITINGS[siting]
    return getattr(fsr.YCbCr, matrix)(full_range=full, siting=code)


def nv12_frame(w, h, k, yc):
    """Frame k of frames.synthetic_frame as NV12 codes: (h, w) Y, ((h + 1) // 2, (w + 1) // 2, 2) Cb, Cr (the mean of each 2 x 2 block)."""
    rgb = frames.synthetic_frame(w, h, k=k, dtype=np.float32)[..., :3].astype(np.float64)
    ycc = (rgb - yc.bias.astype(np.float64)) @ np.linalg.inv(yc.m.astype(np.float64)).T
    c = np.pad(ycc[..., 1:], ((0, h & 1), (0, w & 1), (0, 0)), mode="edge")
    c = c.reshape((h + 1) // 2, 2, (w + 1) // 2, 2, 2).mean(axis=(1, 3))
    return np.clip(np.rint(ycc[..., 0]), 0, 255).astype(np.uint8), np.clip(np.rint(c), 0, 255).astype(np.uint8)


def reference_rgb(y, cbcr, yc):
    """include/fsr1_hip.h, "THE PINNED CONVERSION", in binary32: reconstruct (horizontally, then vertically), convert, clamp."""
    one = np.float32(1)

    def taps(n, cn, mode):  # per position: its own chroma index, the neighbour's (both clamped to the plane), the neighbour's weight
        p = np.arange(n)
        k, o = p >> 1, p & 1
        wgt = {"replicate": 0.0 * o, "cosited": 0.5 * o, "centred": 0.25 + 0.0 * o}[mode].astype(np.float32)
        return np.clip(k, 0, cn - 1), np.clip(k + np.where(o == 1, 1, -1), 0, cn - 1), wgt

    (h, w), (ch, cw), c = y.shape, cbcr.shape[:2], cbcr.astype(np.float32)
    k0, k1, wx = taps(w, cw, ("replicate", "cosited", "centred")[yc.siting])
    j0, j1, wy = taps(h, ch, ("replicate", "centred", "centred")[yc.siting])
    c = (one - wx)[None, :, None] * c[:, k0] + wx[None, :, None] * c[:, k1]
    c = (one - wy)[:, None, None] * c[j0] + wy[:, None, None] * c[j1]
    yf, out = y.astype(np.float32), np.empty((h, w, 3), np.float32)
    for ch_i in range(3):
        v = yc.bias[ch_i] + yc.m[ch_i, 0] * yf
        v = v + yc.m[ch_i, 1] * c[..., 0]
        v = v + yc.m[ch_i, 2] * c[..., 1]
        out[..., ch_i] = np.minimum(np.maximum(v, np.float32(0)), one)
    assert out.dtype == np.float32 and c.dtype == np.float32
    return out


def surface(ys, cs, pitch, chroma_row, rows, poison=0xA5):
    """(N, rows, pitch) device tensor: frame f's Y rows from row 0, its pair rows from row chroma_row, `poison` everywhere else."""
    t = np.full((len(ys), rows, pitch), poison, np.uint8)
    for f, (y, c) in enumerate(zip(ys, cs)):
        t[f, :y.shape[0], :y.shape[1]] = y
        t[f, chroma_row:chroma_row + c.shape[0], :2 * c.shape[1]] = c.reshape(c.shape[0], -1)
    return torch.from_numpy(t).cuda()


@functools.lru_cache(maxsize=None)
def case(shape, siting):
    """What the cases of one shape and siting share: the tight surface, the reference RGB and the oracle's EASU of it, computed once."""
    import cpu_oracle
    port, fsr = cpu_oracle.port(), importlib.import_module("fidelityfx-fsr_amd")
    iw, ih, ow, oh = shape
    yc = ycbcr_of(fsr, siting)
    y, c = nv12_frame(iw, ih, 5, yc)
    rgb = reference_rgb(y, c, yc)
    con = port.FsrEasuCon(iw, ih, iw, ih, ow, oh)
    want = port.easu_f(np.concatenate([rgb, np.ones_like(rgb[..., :1])], -1), ow, oh, con)[..., :3]
    return yc, surface([y], [c], 2 * c.shape[1], ih, ih + c.shape[0])[0, :, :iw], rgb, con, want


def check(dt, got, want, exact, what):
    if dt == "u8":
        check_codes(got, encode(want, 255), exact, what)
    elif exact:
        (assert_exact16 if dt == "f16" else assert_exact32)(got, want, what)
    else:
        assert_f_class(got, want, what)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d_to_%dx%d" % s)
@pytest.mark.parametrize("siting", sorted(SITINGS))
@pytest.mark.parametrize("exact", [True, False], ids=["exact", "default"])
@pytest.mark.parametrize("dt", sorted(OUT))
def test_nv12_easu(fsr, dt, exact, siting, shape):
    yc, src, rgb, con, want = case(shape, siting)
    ow, oh, math = shape[2], shape[3], fsr.FLAG_MATH_EXACT if exact else 0
    out = planes(OUT[dt][0], ow, oh, shape != SHAPES[0])  # the smallest shape in tight rows (element-wise stores), the others padded
    fsr.easu(fsr.Nv12(src), fsr.Planar(out), con=con, flags=math, ycbcr=yc)
    check(dt, to_hwc(out), want, exact, "easu NV12 %s %s" % (siting, dt))
    if dt == "f32":  # the same records as the planar kernel stages from the reference RGB: every bit of the result, both arithmetics
        ref_out = planes(torch.float32, ow, oh, shape != SHAPES[0])
        fsr.easu(fsr.Planar(to_planes(rgb, torch.float32, True)), fsr.Planar(ref_out), con=con, flags=math)
        same_bits(to_hwc(out), to_hwc(ref_out), "NV12 EASU != planar fp32 EASU on the reference RGB (%s)" % siting)


@pytest.mark.parametrize("dt", sorted(OUT))
def test_nv12_batch_on_an_aligned_surface(fsr, port, dt):
    """Three frames, pitch 48 for 37 columns, the pair rows at an aligned height of 16, two spare rows per frame, poison in all the
    padding, EXACT: fsr1_upscale_ycbcr against its two dispatches bit for bit, and against the oracle chain."""
    (tdt, ndt), (iw, ih, ow, oh, n) = OUT[dt], (37, 11, 74, 22, 3)
    yc = ycbcr_of(fsr, "left")
    ys, cs = zip(*(nv12_frame(iw, ih, k, yc) for k in range(n)))
    src = fsr.Nv12(surface(ys, cs, 48, 16, 24)[:, :22, :iw], height=ih)
    assert src.chroma_offset_bytes() == 16 * 48 and src.image().frame_stride_bytes == 24 * 48
    con, rcon = port.FsrEasuCon(iw, ih, iw, ih, ow, oh), port.FsrRcasCon(0.25)
    mid, out, mid2, out2 = (planes(tdt, ow, oh, True, n) for _ in range(4))
    fsr.upscale_ycbcr(src, fsr.Planar(mid), fsr.Planar(out), yc, sharpness=0.25, fused=2, flags=fsr.FLAG_MATH_EXACT)
    fsr.easu(src, fsr.Planar(mid2), con=con, flags=fsr.FLAG_MATH_EXACT, ycbcr=yc)
    fsr.rcas(fsr.Planar(mid2), fsr.Planar(out2), con=rcon, flags=fsr.FLAG_MATH_EXACT)
    got = to_hwc(out)
    same_bits(got, to_hwc(out2), "fsr1_upscale_ycbcr != easu_dispatch_ycbcr -> rcas")
    for k in range(n):
        rgb = reference_rgb(ys[k], cs[k], yc)
        want_mid = port.easu_f(np.concatenate([rgb, np.ones_like(rgb[..., :1])], -1), ow, oh, con)
        want_mid = decode(encode(want_mid, 255), 255) if dt == "u8" else want_mid.astype(ndt).astype(np.float32)  # stored: the plane's type
        want_mid[..., 3] = 1
        check(dt, got[k], port.rcas_f(want_mid, rcon)[..., :3], True, "chain EXACT NV12 frame %d" % k)


def _params(F, use_rcas=1, fused=0, flags=0):
    return ctypes.byref(F.fsr1_params(8.0, 8.0, use_rcas, 0.25, 0, fused, flags))


def _stage(F):
    return ctypes.byref(F.fsr1_color_stages(F.COLOR_SRTM, 0, 0, 0, 0, 0, None))


def _pipeline(L, F, n, o):
    p = F.Pipeline(1)
    try:
        return L.fsr1_pipeline_upscale(p._h, n, o, _params(F), None)
    finally:
        p.close()


# n: an NV12 image, o / o2: planar fp16 images of twice the size, r: an RGBA16F one, y / bad: fsr1_ycbcr with a known / unknown siting
REFUSED = {
    "easu_dispatch": lambda L, F, n, o, o2, r, c, rc, y, bad: L.fsr1_easu_dispatch(n, o, c, 0, None),
    "easu_dispatch_ex": lambda L, F, n, o, o2, r, c, rc, y, bad: L.fsr1_easu_dispatch_ex(n, o, c, 0, _stage(F), None),
    "rcas_dispatch": lambda L, F, n, o, o2, r, c, rc, y, bad: L.fsr1_rcas_dispatch(n, n, rc, 0, None),
    "fused_dispatch": lambda L, F, n, o, o2, r, c, rc, y, bad: L.fsr1_easu_rcas_fused_dispatch(n, r, c, rc, 0, None),
    "easu_band": lambda L, F, n, o, o2, r, c, rc, y, bad: L.fsr1_easu_dispatch_band(n, o, c, 0, 0, 0, None),
    "color_dispatch": lambda L, F, n, o, o2, r, c, rc, y, bad: L.fsr1_color_dispatch(n, n, _stage(F), 0, None),
    "upscale": lambda L, F, n, o, o2, r, c, rc, y, bad: L.fsr1_upscale(n, o2, o, _params(F), None),
    "upscale_plan": lambda L, F, n, o, o2, r, c, rc, y, bad: L.fsr1_upscale_plan(n, 1, o, _params(F), 0),
    "pipeline": lambda L, F, n, o, o2, r, c, rc, y, bad: _pipeline(L, F, n, o),
    "nv12_output": lambda L, F, n, o, o2, r, c, rc, y, bad: L.fsr1_easu_dispatch_ycbcr(n, n, c, y, 0, None),
    "interleaved_output": lambda L, F, n, o, o2, r, c, rc, y, bad: L.fsr1_easu_dispatch_ycbcr(n, r, c, y, 0, None),
    "planar_input": lambda L, F, n, o, o2, r, c, rc, y, bad: L.fsr1_easu_dispatch_ycbcr(o2, o, c, y, 0, None),
    "packed_fp16": lambda L, F, n, o, o2, r, c, rc, y, bad: L.fsr1_easu_dispatch_ycbcr(n, o, c, y, F.FLAG_MATH_PACKED_FP16, None),
    "unknown_siting": lambda L, F, n, o, o2, r, c, rc, y, bad: L.fsr1_easu_dispatch_ycbcr(n, o, c, bad, 0, None),
    "fused_1": lambda L, F, n, o, o2, r, c, rc, y, bad: L.fsr1_upscale_ycbcr(n, o2, o, _params(F, fused=1), y, None),
    "no_intermediary": lambda L, F, n, o, o2, r, c, rc, y, bad: L.fsr1_upscale_ycbcr(n, None, o, _params(F, fused=2), y, None),
}


@pytest.mark.parametrize("what", sorted(REFUSED))
def test_nv12_refusals(fsr, what):
    lib = fsr.load()
    z = lambda *s: torch.zeros(*s, dtype=torch.float16, device="cuda")  # noqa: E731
    imgs = (fsr.Nv12(torch.zeros(12, 8, dtype=torch.uint8, device="cuda")), fsr.Planar(z(3, 16, 16)), fsr.Planar(z(3, 16, 16)), z(16, 16, 4))
    n, o, o2, r = (ctypes.byref(fsr.image_of(t)) for t in imgs)
    y, bad = (ctypes.byref(fsr.YCbCr.bt601(siting=s).c_struct()) for s in (1, 3))
    cons = (a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)) for a in (fsr.FsrEasuCon(8, 8, 8, 8, 16, 16), fsr.FsrRcasCon(0.25)))
    assert REFUSED[what](lib, fsr, n, o, o2, r, *cons, y, bad) == -2
    assert b"NV12" in lib.fsr1_last_error(), lib.fsr1_last_error()


@pytest.mark.parametrize("t,height", [(lambda: torch.zeros(12, 8, dtype=torch.float16, device="cuda"), None),  # not uint8
                                      (lambda: torch.zeros(12, 8, dtype=torch.uint8, device="cuda"), 9),      # 9 + 5 rows do not fit 12
                                      (lambda: torch.zeros(5, 5, dtype=torch.uint8, device="cuda"), None),    # 5 bytes hold no 3 pairs
                                      (lambda: torch.zeros(2, 3, 12, 8, dtype=torch.uint8, device="cuda"), None)],
                         ids=["float16", "too_tall", "odd_width_tight", "four_dims"])
def test_nv12_surface_validation(fsr, t, height):
    with pytest.raises(fsr.Fsr1Error):
        fsr.image_of(fsr.Nv12(t(), height=height))
