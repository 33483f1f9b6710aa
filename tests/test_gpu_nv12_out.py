"""RCAS straight into an NV12 surface (rcas(src, Nv12(dst), ycbcr=RgbToYCbCr), fsr1_rcas_dispatch_ycbcr) and the NV12 -> NV12 chain
(transcode_ycbcr).  The reference is reference_nv12(): "THE PINNED CONVERSION, RGB -> NV12" of include/fsr1_hip.h restated in numpy
float32, applied to the planar binary32 RCAS result of the same input and flags (both kernels call the same rcas_pixel, so every code
must be EQUAL in both arithmetics — a contracted multiply-add in the conversion shows here) and, EXACT, to the CPU oracle's."""
import ctypes
import functools
import importlib
import itertools

import numpy as np
import pytest

from test_gpu_nv12 import nv12_frame, reference_rgb, surface, ycbcr_of
from test_gpu_planar import planes, to_hwc, to_planes
from test_gpu_unorm import decode, encode

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
frames = importlib.import_module("fidelityfx-fsr_amd.frames")

POISON = 0xA5
IN = {"f16": (torch.float16, np.float16), "f32": (torch.float32, np.float32), "u8": (torch.uint8, np.uint8)}
SITINGS = {"center": (2, "bt709", False), "replicate": (0, "bt601", True)}  # siting -> (code, the matrix it is tested with, full range)
# (W, H) -> row pitch of the surface.  5 x 3: odd both ways, one ragged lane, tight rows (element-wise stores) | 515 x 35: 8-row strips
# walking down and up, the x-edge body, an interior second wave, a second workgroup of three columns ending on a lone odd column, an odd
# last row that pairs with itself; the pitch is even only: bytes and 16-bit pairs in every body | 600 x 40: dword stores throughout
SHAPES = {(5, 3): 6, (515, 35): 518, (600, 40): 608}
CASES = [c + (0,) for c in itertools.product(SHAPES, sorted(SITINGS), [True, False], sorted(IN))] + \
        [((515, 35), "center", True, "f32", "FLAG_RCAS_DENOISE"), ((600, 40), "replicate", True, "f16", "FLAG_HDR_SQUARE")]


def conv_of(fsr, siting):
    code, matrix, full = SITINGS[siting]
    return getattr(fsr.RgbToYCbCr, matrix)(full_range=full, siting=code)


def reference_nv12(rgb32, conv):
    """include/fsr1_hip.h, "THE PINNED CONVERSION, RGB -> NV12", in binary32: (h, w) Y codes and ((h + 1) // 2, (w + 1) // 2, 2) pairs."""
    assert rgb32.dtype == np.float32 and conv.m.dtype == np.float32
    h, w = rgb32.shape[:2]

    def codes(k, p):
        v = conv.bias[k] + conv.m[k, 0] * p[..., 0]
        v = v + conv.m[k, 1] * p[..., 1]
        v = v + conv.m[k, 2] * p[..., 2]
        v = np.where(np.isnan(v), np.float32(0), v)
        v = np.minimum(np.maximum(v, np.float32(0)), np.float32(255)) + np.float32(0.5)
        assert v.dtype == np.float32
        return v.astype(np.uint8)  # truncation

    x0, y0 = np.arange(0, w, 2), np.arange(0, h, 2)
    x1, y1 = np.minimum(x0 + 1, w - 1), np.minimum(y0 + 1, h - 1)
    if conv.siting == 2:
        s0, s1 = rgb32[y0][:, x0] + rgb32[y0][:, x1], rgb32[y1][:, x0] + rgb32[y1][:, x1]
        a = np.float32(0.25) * (s0 + s1)
    else:
        a = rgb32[y0][:, x0]
    return codes(0, rgb32), np.stack([codes(1, a), codes(2, a)], -1)


def split(surf, w, h, chroma_row):
    """A host (rows, pitch) surface -> its Y codes, its pairs, and a copy with both regions poisoned again (the padding's view)."""
    cw, ch = (w + 1) // 2, (h + 1) // 2
    y, c = surf[:h, :w].copy(), surf[chroma_row:chroma_row + ch, :2 * cw].reshape(ch, cw, 2).copy()
    rest = surf.copy()
    rest[:h, :w] = POISON
    rest[chroma_row:chroma_row + ch, :2 * cw] = POISON
    return y, c, rest


@functools.lru_cache(maxsize=None)
def source(shape, dt):
    """The input of one shape and type as host values of that type, and decoded to the binary32 the kernels filter."""
    rgb = frames.synthetic_frame(shape[0], shape[1], k=5, dtype=np.float32)[..., :3]
    if dt == "u8":
        stored = encode(rgb, 255).astype(np.uint8)
        return stored, decode(stored, 255)
    stored = rgb.astype(IN[dt][1])
    return stored, stored.astype(np.float32)


@pytest.mark.parametrize("shape,siting,exact,dt,opt", CASES, ids=lambda v: "%dx%d" % v if isinstance(v, tuple) else str(v))
def test_rcas_to_nv12(fsr, port, shape, siting, exact, dt, opt):
    (w, h), pitch, ch = shape, SHAPES[shape], (shape[1] + 1) // 2
    opts = getattr(fsr, opt) if opt else 0
    flags, conv, rcon = (fsr.FLAG_MATH_EXACT if exact else 0) | opts, conv_of(fsr, siting), port.FsrRcasCon(0.25)
    stored, rgb32 = source(shape, dt)
    dst = torch.full((h + ch, pitch), POISON, dtype=torch.uint8, device="cuda")
    fsr.rcas(fsr.Planar(to_planes(stored, IN[dt][0], shape != (5, 3))), fsr.Nv12(dst[:, :w]), con=rcon, flags=flags, ycbcr=conv)
    ref_out = planes(torch.float32, w, h, True)
    fsr.rcas(fsr.Planar(to_planes(rgb32, torch.float32, True)), fsr.Planar(ref_out), con=rcon, flags=flags)
    got_y, got_c, rest = split(dst.cpu().numpy(), w, h, h)
    assert (rest == POISON).all(), "bytes outside the Y and pair regions were written"
    wants = [("the planar fp32 RCAS", to_hwc(ref_out))]
    if exact:
        oracle_flags = (1 if opts & fsr.FLAG_RCAS_DENOISE else 0) | (4 if opts & fsr.FLAG_HDR_SQUARE else 0)
        wants.append(("the oracle's rcas_f", port.rcas_f(np.concatenate([rgb32, np.ones_like(rgb32[..., :1])], -1), rcon, oracle_flags)[..., :3]))
    for name, rgb in wants:
        want_y, want_c = reference_nv12(np.ascontiguousarray(rgb, np.float32), conv)
        assert np.array_equal(got_y, want_y), "Y != reference_nv12 of %s: %d codes differ" % (name, (got_y != want_y).sum())
        assert np.array_equal(got_c, want_c), "CbCr != reference_nv12 of %s: %d codes differ" % (name, (got_c != want_c).sum())


def test_transcode_batch(fsr, port):
    """Three frames of 37 x 11 -> 74 x 22, padded pitches, the pair rows at aligned heights on both surfaces, poison in all the
    padding, EXACT: fsr1_transcode_ycbcr against its two dispatches bit for bit, and against the oracle chain."""
    iw, ih, ow, oh, n = 37, 11, 74, 22, 3
    yc, conv = ycbcr_of(fsr, "left"), conv_of(fsr, "center")
    ys, cs = zip(*(nv12_frame(iw, ih, k, yc) for k in range(n)))
    src = fsr.Nv12(surface(ys, cs, 48, 16, 24)[:, :22, :iw], height=ih)
    con, rcon = port.FsrEasuCon(iw, ih, iw, ih, ow, oh), port.FsrRcasCon(0.25)
    dst, dst2 = (torch.full((n, 48, 80), POISON, dtype=torch.uint8, device="cuda") for _ in range(2))  # Y rows 0 .. 21, pairs from row 32, 5 spare
    out, out2 = (fsr.Nv12(t[:, :43, :ow], height=oh) for t in (dst, dst2))
    assert out.chroma_offset_bytes() == 32 * 80 and out.image().frame_stride_bytes == 48 * 80
    mid, mid2 = (planes(torch.float16, ow, oh, True, n) for _ in range(2))
    fsr.transcode_ycbcr(src, fsr.Planar(mid), out, yc, conv, sharpness=0.25, fused=2, flags=fsr.FLAG_MATH_EXACT)
    fsr.easu(src, fsr.Planar(mid2), con=con, flags=fsr.FLAG_MATH_EXACT, ycbcr=yc)
    fsr.rcas(fsr.Planar(mid2), out2, con=rcon, flags=fsr.FLAG_MATH_EXACT, ycbcr=conv)
    got = dst.cpu().numpy()
    assert np.array_equal(got, dst2.cpu().numpy()), "fsr1_transcode_ycbcr != easu_dispatch_ycbcr -> rcas_dispatch_ycbcr"
    for k in range(n):
        rgb = reference_rgb(ys[k], cs[k], yc)
        want_mid = port.easu_f(np.concatenate([rgb, np.ones_like(rgb[..., :1])], -1), ow, oh, con).astype(np.float16).astype(np.float32)
        want_mid[..., 3] = 1
        want_y, want_c = reference_nv12(np.ascontiguousarray(port.rcas_f(want_mid, rcon)[..., :3], np.float32), conv)
        got_y, got_c, rest = split(got[k], ow, oh, 32)
        assert (rest == POISON).all(), "frame %d: padding written" % k
        assert np.array_equal(got_y, want_y) and np.array_equal(got_c, want_c), "frame %d != the oracle chain" % k


def _params(F, use_rcas=1, fused=0):
    return ctypes.byref(F.fsr1_params(8.0, 8.0, use_rcas, 0.25, 0, fused, 0))


# n / N: NV12 images of 8 x 8 / 16 x 16, p / p2: planar fp16 images of 16 x 16, r: an RGBA16F one, c: a conversion by its siting
REFUSED = {
    "interleaved_input": lambda L, F, n, N, p, p2, r, rc, yi, c: L.fsr1_rcas_dispatch_ycbcr(r, N, rc, c(2), 0, None),
    "nv12_input": lambda L, F, n, N, p, p2, r, rc, yi, c: L.fsr1_rcas_dispatch_ycbcr(N, N, rc, c(2), 0, None),
    "planar_output": lambda L, F, n, N, p, p2, r, rc, yi, c: L.fsr1_rcas_dispatch_ycbcr(p, p2, rc, c(2), 0, None),
    "packed_fp16": lambda L, F, n, N, p, p2, r, rc, yi, c: L.fsr1_rcas_dispatch_ycbcr(p, N, rc, c(2), F.FLAG_MATH_PACKED_FP16, None),
    "passthrough_alpha": lambda L, F, n, N, p, p2, r, rc, yi, c: L.fsr1_rcas_dispatch_ycbcr(p, N, rc, c(2), F.FLAG_RCAS_PASSTHROUGH_ALPHA, None),
    "siting_left": lambda L, F, n, N, p, p2, r, rc, yi, c: L.fsr1_rcas_dispatch_ycbcr(p, N, rc, c(1), 0, None),
    "unknown_siting": lambda L, F, n, N, p, p2, r, rc, yi, c: L.fsr1_rcas_dispatch_ycbcr(p, N, rc, c(3), 0, None),
    "use_rcas_0": lambda L, F, n, N, p, p2, r, rc, yi, c: L.fsr1_transcode_ycbcr(n, p, N, _params(F, use_rcas=0), yi, c(2), None),
    "fused_1": lambda L, F, n, N, p, p2, r, rc, yi, c: L.fsr1_transcode_ycbcr(n, p, N, _params(F, fused=1), yi, c(2), None),
    "no_intermediary": lambda L, F, n, N, p, p2, r, rc, yi, c: L.fsr1_transcode_ycbcr(n, None, N, _params(F, fused=2), yi, c(2), None),
}
INVALID = {
    "overlap": lambda L, F, p, N, odd, rc, c: L.fsr1_rcas_dispatch_ycbcr(p, F.fsr1_image(p.data, 16, 16, F.FORMAT_NV12, 1, 0, 0), rc, c(2), 0, None),
    "odd_pitch": lambda L, F, p, N, odd, rc, c: L.fsr1_rcas_dispatch_ycbcr(p, odd, rc, c(2), 0, None),
}


@pytest.mark.parametrize("what", sorted(REFUSED) + sorted(INVALID))
def test_nv12_out_refusals(fsr, what):
    lib = fsr.load()
    z = lambda *s, dt=torch.float16: torch.zeros(*s, dtype=dt, device="cuda")  # noqa: E731
    imgs = [fsr.image_of(t) for t in (fsr.Nv12(z(12, 8, dt=torch.uint8)), fsr.Nv12(z(24, 16, dt=torch.uint8)), fsr.Planar(z(3, 16, 16)),
                                      fsr.Planar(z(3, 16, 16)), z(16, 16, 4))]
    n, N, p, p2, r = imgs
    odd = fsr.fsr1_image(N.data, 16, 16, fsr.FORMAT_NV12, 1, 17, 0)
    rc = fsr.FsrRcasCon(0.25).ctypes.data_as(ctypes.POINTER(ctypes.c_uint32))
    yi = ctypes.byref(fsr.YCbCr.bt601().c_struct())
    c = lambda s: ctypes.byref(fsr.RgbToYCbCr.bt601(siting=s).c_struct())  # noqa: E731
    if what in REFUSED:
        assert REFUSED[what](lib, fsr, *(ctypes.byref(i) for i in imgs), rc, yi, c) == -2
        assert b"NV12" in lib.fsr1_last_error(), lib.fsr1_last_error()
    else:
        assert INVALID[what](lib, fsr, p, N, odd, rc, c) == -1, lib.fsr1_last_error()
