"""The luma-domain NV12 transcode (transcode_luma, fsr1_transcode_luma): the Y plane must be, bit for bit, what the single-channel
EASU -> RCAS chain stores on views of the same memory (and, EXACT, the CPU oracle's), the pair plane the numpy float32 restatement of
"THE PINNED LUMA-DOMAIN TRANSCODE" (include/fsr1_hip.h), and nothing else of the surface may be written.  Every comparison is equality."""
import ctypes
import functools
import importlib

import numpy as np
import pytest

from test_gpu_mono import as_f32, check, plane, rgba
from test_gpu_nv12 import nv12_frame, surface, ycbcr_of
from test_gpu_nv12_out import POISON, split
from test_gpu_planar import same_bits
from test_gpu_unorm import encode

torch = pytest.importorskip("torch")

LEFT, CENTER = 1, 2
# (iw, ih, ow, oh) -> (input pitch, output pitch).  5x3: odd both ways, one ragged lane, tight Y rows, 16-bit loads and stores, generic
# ratio | 66x19: exact 2x, the EASU tile seam at column 64, an odd input height, dword loads, 8-byte stores | 345x23: 259 output pairs,
# three more than a wave's 256 (a wave seam and a lane the edge cuts), an odd last row, pitch padded to 8 | 131x83: minification, j0
# advances by more than one per output row, 16-bit loads
SHAPES = {(5, 3, 17, 9): (6, 18), (66, 19, 132, 38): (68, 136), (345, 23, 518, 35): (348, 520), (131, 83, 97, 61): (132, 98)}
SITINGS = [(LEFT, LEFT), (CENTER, LEFT), (LEFT, CENTER)]


def reference_chroma(c, CW, CH, render, out, s_in, s_out):
    """include/fsr1_hip.h, "THE PINNED LUMA-DOMAIN TRANSCODE", chroma, in binary32: (ch, cw, 2) codes -> (CH, CW, 2) codes."""
    def axis(n_out, n_in, r, o, si, so):
        scale = r / o                                    # double
        off = ((so + 0.5) * scale - 0.5 - si) / 2
        u = np.arange(n_out, dtype=np.float32) * np.float32(scale) + np.float32(off)
        k0 = np.floor(u)
        assert u.dtype == np.float32
        return np.clip(k0.astype(np.int64), 0, n_in - 1), np.clip(k0.astype(np.int64) + 1, 0, n_in - 1), u - k0

    c = c.astype(np.float32)
    ka, kb, f = axis(CW, c.shape[1], render[0], out[0], 0.5 * (s_in == CENTER), 0.5 * (s_out == CENTER))
    ja, jb, g = axis(CH, c.shape[0], render[1], out[1], 0.5, 0.5)
    h = c[:, ka] + f[None, :, None] * (c[:, kb] - c[:, ka])
    v = h[ja] + g[:, None, None] * (h[jb] - h[ja])
    v = np.minimum(np.maximum(v, np.float32(0)), np.float32(255)) + np.float32(0.5)
    assert v.dtype == np.float32
    return v.astype(np.uint8)  # truncation


@functools.lru_cache(maxsize=None)
def luma_case(shape, exact, render=None):
    """What the sitings of one shape and arithmetic share: the source frame and surface, and the Y plane the two single-channel
    dispatches store on views of a second surface (checked against the oracle chain under EXACT), computed once."""
    import cpu_oracle
    port, fsr = cpu_oracle.port(), importlib.import_module("fidelityfx-fsr_amd")
    (iw, ih, ow, oh), (ip, op) = shape, SHAPES[shape]
    rw, rh = render or (iw, ih)
    y, c = nv12_frame(iw, ih, 5, ycbcr_of(fsr, "left"))
    src = surface([y], [c], ip, ih, ih + c.shape[0])[0]
    flags, con, rcon = fsr.FLAG_MATH_EXACT if exact else 0, port.FsrEasuCon(rw, rh, rw, rh, ow, oh), port.FsrRcasCon(0.25)
    mid, ref = plane(torch.uint8, ow, oh, op % 4 == 0), torch.full((oh, op), POISON, dtype=torch.uint8, device="cuda")
    fsr.easu(fsr.Mono(src[:ih, :iw]), fsr.Mono(mid), con=con, flags=flags)
    fsr.rcas(fsr.Mono(mid), fsr.Mono(ref[:, :ow]), con=rcon, flags=flags)
    want_y = ref.cpu().numpy()[:, :ow]
    if exact:
        want_mid = port.easu_f(as_f32("u8", rgba("u8", y)), ow, oh, con)[..., 0]
        want_mid = encode(want_mid, 255).astype(np.uint8)  # stored: rounded to codes
        check("u8", want_y, port.rcas_f(as_f32("u8", rgba("u8", want_mid)), rcon), True, "the single-channel chain against the oracle")
    return c, src, want_y


def run(fsr, shape, exact, sitings, render=None):
    (iw, ih, ow, oh), (ip, op) = shape, SHAPES[shape]
    c, src, want_y = luma_case(shape, exact, render)
    CW, CH = (ow + 1) // 2, (oh + 1) // 2
    dst = torch.full((oh + CH, op), POISON, dtype=torch.uint8, device="cuda")
    mid = plane(torch.uint8, ow, oh, op % 4 == 0)
    fsr.transcode_luma(fsr.Nv12(src[:, :iw], height=ih), fsr.Mono(mid), fsr.Nv12(dst[:, :ow], height=oh), siting_in=sitings[0], siting_out=sitings[1],
                       sharpness=0.25, flags=fsr.FLAG_MATH_EXACT if exact else 0, render_size=render)
    got_y, got_c, rest = split(dst.cpu().numpy(), ow, oh, oh)
    assert (rest == POISON).all(), "bytes outside the Y and pair regions were written"
    same_bits(got_y, want_y, "Y plane != easu(Mono) -> rcas(Mono) on views of the same memory")
    want_c = reference_chroma(c, CW, CH, render or (iw, ih), (ow, oh), *sitings)
    assert np.array_equal(got_c, want_c), "pair plane != the float32 restatement: %d codes differ" % (got_c != want_c).sum()


@pytest.mark.gpu
@pytest.mark.parametrize("sitings", SITINGS, ids=["left_left", "center_left", "left_center"])
@pytest.mark.parametrize("exact", [False, True], ids=["default", "exact"])
@pytest.mark.parametrize("shape", sorted(SHAPES), ids=lambda s: "%dx%d_to_%dx%d" % s)
def test_luma_transcode(fsr, shape, exact, sitings):
    run(fsr, shape, exact, sitings)


@pytest.mark.gpu
def test_luma_transcode_render_size(fsr):
    """A render size smaller than the input resource: the constants of both planes come from it, the clamps from the resource."""
    run(fsr, (66, 19, 132, 38), True, (LEFT, LEFT), render=(60, 16))


@pytest.mark.gpu
def test_luma_batch(fsr):
    """Three frames of 37 x 11 -> 74 x 22, padded pitches, the pair rows at an aligned height on both surfaces, EXACT: each frame equals
    the single-frame call, and no padding is written."""
    iw, ih, ow, oh, n = 37, 11, 74, 22, 3
    ys, cs = zip(*(nv12_frame(iw, ih, k, ycbcr_of(fsr, "left")) for k in range(n)))
    src = surface(ys, cs, 48, 16, 24)[:, :22, :iw]
    dst = torch.full((n, 48, 80), POISON, dtype=torch.uint8, device="cuda")  # Y rows 0 .. 21, pairs from row 32, 5 spare
    fsr.transcode_luma(fsr.Nv12(src, height=ih), fsr.Mono(plane(torch.uint8, ow, oh, True, n)), fsr.Nv12(dst[:, :43, :ow], height=oh), CENTER, LEFT,
                       flags=fsr.FLAG_MATH_EXACT)
    for k in range(n):
        one = torch.full((48, 80), POISON, dtype=torch.uint8, device="cuda")
        fsr.transcode_luma(fsr.Nv12(src[k], height=ih), fsr.Mono(plane(torch.uint8, ow, oh, True)), fsr.Nv12(one[:43, :ow], height=oh), CENTER, LEFT,
                           flags=fsr.FLAG_MATH_EXACT)
        same_bits(dst[k].cpu().numpy(), one.cpu().numpy(), "frame %d of the batch != the single-frame call" % k)
        got_y, got_c, rest = split(one.cpu().numpy(), ow, oh, 32)
        assert (rest == POISON).all() and (got_y != POISON).any() and np.array_equal(got_c, reference_chroma(cs[k], 37, 11, (iw, ih), (ow, oh), CENTER, LEFT))


def _call(L, F, i, m, o, use_rcas=1, hdr=0, fused=0, flags=0, sitings=(LEFT, LEFT), render=(8.0, 8.0)):
    return L.fsr1_transcode_luma(i, m, o, ctypes.byref(F.fsr1_params(render[0], render[1], use_rcas, 0.25, hdr, fused, flags)),
                                 ctypes.byref(F.fsr1_chroma420(sitings[0], sitings[1], 0, 0)), None)


# n / N: NV12 images of 8 x 8 / 16 x 16, m: an R8_UNORM image of 16 x 16; img(format, size, frames, address) makes the others
REFUSED = {
    "p010_in": lambda L, F, n, m, N, img: _call(L, F, img(F.FORMAT_P010, 8), m, N),
    "p016_out": lambda L, F, n, m, N, img: _call(L, F, n, m, img(F.FORMAT_P016, 16)),
    "intermediary_not_r8": lambda L, F, n, m, N, img: _call(L, F, n, img(F.FORMAT_R16F, 16), N),
    "fused_1": lambda L, F, n, m, N, img: _call(L, F, n, m, N, fused=1),
    "use_rcas_0": lambda L, F, n, m, N, img: _call(L, F, n, m, N, use_rcas=0),
    "no_intermediary": lambda L, F, n, m, N, img: _call(L, F, n, None, N, fused=2),
    "packed_fp16": lambda L, F, n, m, N, img: _call(L, F, n, m, N, flags=F.FLAG_MATH_PACKED_FP16),
    "siting_replicate": lambda L, F, n, m, N, img: _call(L, F, n, m, N, sitings=(0, LEFT)),
    "siting_unknown": lambda L, F, n, m, N, img: _call(L, F, n, m, N, sitings=(LEFT, 3)),
}
INVALID = {
    "null": lambda L, F, n, m, N, img: L.fsr1_transcode_luma(n, m, N, None, None, None),
    "hdr": lambda L, F, n, m, N, img: _call(L, F, n, m, N, hdr=1),
    "extents": lambda L, F, n, m, N, img: _call(L, F, n, img(F.FORMAT_R8_UNORM, 12), N),
    "frames": lambda L, F, n, m, N, img: _call(L, F, img(F.FORMAT_NV12, 8, 2), m, N),
    "render_size": lambda L, F, n, m, N, img: _call(L, F, n, m, N, render=(9.0, 8.0)),
    "overlap": lambda L, F, n, m, N, img: _call(L, F, n, img(F.FORMAT_R8_UNORM, 16, 1, 0x200100), N),
    "unknown_flag": lambda L, F, n, m, N, img: _call(L, F, n, m, N, flags=1 << 12),
}


@pytest.mark.parametrize("what", [pytest.param(w, marks=() if w == "null" else pytest.mark.gpu) for w in sorted(REFUSED) + sorted(INVALID)])
def test_luma_refusals(fsr, what):
    """Every refusal is made before anything is launched or dereferenced: the descriptors carry addresses of no allocation."""
    lib = fsr.load()
    img = lambda fmt, size, frames=1, addr=0x400000: ctypes.byref(fsr.fsr1_image(addr, size, size, fmt, frames, 0, 0))  # noqa: E731
    n, m, N = img(fsr.FORMAT_NV12, 8, 1, 0x100000), img(fsr.FORMAT_R8_UNORM, 16, 1, 0x300000), img(fsr.FORMAT_NV12, 16, 1, 0x200000)
    if what in REFUSED:
        assert REFUSED[what](lib, fsr, n, m, N, img) == -2
        assert b"NV12" in lib.fsr1_last_error(), lib.fsr1_last_error()
    else:
        assert INVALID[what](lib, fsr, n, m, N, img) == -1, lib.fsr1_last_error()
