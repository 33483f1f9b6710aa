"""Class H (packed binary16) colour stages fused into EASU-H and RCAS-H, the RGBA16F -> 32 bpp UNORM RCAS-H kernel, the two-dispatch
class-H chain with stages and the stand-alone H colour pass on every class-H format.  The reference value is the CPU oracle composed
stage by stage — enc_out(color_h(rcas_h(color_h(dec_in(x), SRTM)), epilogue)), easu_h in front for the chains — whose H entry points
narrow their input RTNE (TexelH's load rule), so the composition is exact and every assertion is "0 bits / codes differ".
Where FsrSrtmH leads, RGBA16F inputs are HDR (up to 16), set A (SRTM_INV straight after the sharpened SRTM image) included: the seeds
below give an all-finite-or-infinite oracle image (no NaN), which every case asserts as its precondition."""
import ctypes

import numpy as np
import pytest

from test_gpu_color import dev, host, stages_of
from test_gpu_unorm_h import FORMATS, same

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


class F16:
    dec = staticmethod(lambda a: a.astype(np.float32))
    enc = staticmethod(lambda x: np.asarray(x, np.float32).astype(np.float16))
    up = staticmethod(dev)
    host = staticmethod(host)
    empty = staticmethod(lambda *lead: torch.zeros(*lead, 4, dtype=torch.float16, device="cuda"))


FMT = dict(FORMATS, f16=F16)
H_STAGES = (1 << 5) | (1 << 7)  # FSR1_FLAG_MATH_PACKED_FP16 | FSR1_FLAG_COLOR_STAGES_H: the filters and their colour stages in class H
SETS = {"A": 1 | 4, "B": 1 | 2 | 8, "C": 2 | 16 | 32}  # SRTM | SRTM_INV ; SRTM | LFGA | TEPD_C8 ; LFGA | TEPD_C10 | DITHER_FROM_NOISE
P = dict(amount=0.5, bias=0.0, frame=3, noise_offset=(-3, 5))
_rng = np.random.default_rng(11)  # a 16 x 8 tile (it wraps), two slices, binary16: grain in RGB, dither in A
NOISE = (_rng.random((2, 8, 16, 4)).astype(np.float32) - np.array([0.5, 0.5, 0.5, 0.0], np.float32)).astype(np.float16)


def source(fmt, w, h, st, seed, n=None):
    """Stored image(s) in `fmt`: HDR values (up to 16) in RGBA16F where SRTM leads, otherwise values inside 0 .. 1."""
    img = np.random.default_rng(seed).random((h, w, 4) if n is None else (n, h, w, 4)).astype(np.float32)
    if fmt == "f16" and st & 1:
        img[..., :3] = img[..., :3] ** 2 * 16.0
    return FMT[fmt].enc(img)


def oracle(port, x, st, fin="f16", easu=None, rcon=None, rflags=0):
    """The chain on one decoded frame: SRTM, EASU (the intermediary stored in `fin`), RCAS, the epilogue."""
    x = port.color_h(x, 1) if st & 1 else x
    if easu is not None:
        x = port.easu_h(x, *easu)
        x = FMT[fin].dec(FMT[fin].enc(x)) if rcon is not None else x
    x = port.rcas_h(x, rcon, rflags) if rcon is not None else x
    x = port.color_h(x, st & ~1, noise=NOISE.astype(np.float32), **P) if st & ~1 else x
    assert not np.isnan(x).any(), "precondition: the oracle image holds a NaN"
    return x


def bits(a):
    return a.view(np.uint16) if a.dtype == np.float16 else a


def check(fmt, got_t, want, what):
    same(bits(FMT[fmt].host(got_t)), bits(FMT[fmt].enc(want)), what)


def plan(fsr, iw, ih, ow, oh, fin, fout, use_rcas, fused):
    code = {"f16": 0, "rgba8": 2, "rgb10a2": 3}
    a, b = fsr.fsr1_image(0x1000, iw, ih, code[fin], 1, 0, 0), fsr.fsr1_image(0x10000000, ow, oh, code[fout], 1, 0, 0)
    prm = fsr._lib.fsr1_params(float(iw), float(ih), use_rcas, 0.25, 0, fused, H_STAGES)
    return fsr.load().fsr1_upscale_plan(ctypes.byref(a), 1, ctypes.byref(b), ctypes.byref(prm), 1)


RCAS_CASES = [(f, f, s) for f in ("f16", "rgba8", "rgb10a2") for s in "ABC"] + [("f16", "rgba8", "B"), ("f16", "rgb10a2", "C")]


@pytest.mark.parametrize("fin,fout,sset", RCAS_CASES, ids=lambda v: str(v))
def test_rcas_h_stages(fsr, port, fin, fout, sset):
    """515 x 17: the wave seam at column 256, the workgroup seam at 512, width mod 4 = 3, three 8-row strips."""
    st, (w, h) = SETS[sset], (515, 17)
    x = source(fin, w, h, st, 7)
    rcon = port.FsrRcasCon(0.25)
    out = FMT[fout].empty(h, w)
    fsr.rcas(FMT[fin].up(x), out, con=rcon, flags=H_STAGES, stages=stages_of(fsr, st, dev(NOISE), P))
    check(fout, out, oracle(port, FMT[fin].dec(x), st, rcon=rcon), "rcas H %s -> %s, set %s" % (fin, fout, sset))


def test_rcas_h_to_rgba8_narrow_with_options(fsr, port):
    """5 x 3 (narrower than the second lane's four pixels), denoise + alpha pass-through + `c *= c`, an alpha ramp."""
    w, h, st = 5, 3, SETS["B"]
    x = source("f16", w, h, st, 3)
    x[..., 3] = ((np.arange(w)[None, :] + np.arange(h)[:, None]) / 7.0).astype(np.float16)
    rcon = port.FsrRcasCon(0.25)
    out = FMT["rgba8"].empty(h, w)
    flags = H_STAGES | fsr.FLAG_RCAS_DENOISE | fsr.FLAG_RCAS_PASSTHROUGH_ALPHA | fsr.FLAG_HDR_SQUARE
    fsr.rcas(dev(x), out, con=rcon, flags=flags, stages=stages_of(fsr, st, dev(NOISE), P))
    check("rgba8", out, oracle(port, x.astype(np.float32), st, rcon=rcon, rflags=1 | 2 | 4), "rcas H -> rgba8, options")


def upscale(fsr, src, dst, iw, ih, ow, oh, use_rcas, fused, st):
    filt = fsr.FSR_Filter()
    filt.OnCreate(slowFallback=False, fused=fused)
    filt.OnCreateWindowSizeDependentResources(src, dst, ow, oh)
    filt.Upscale(ow, oh, fsr.State(iw, ih, bUseRcas=use_rcas, rcasAttenuation=0.25), stages=stages_of(fsr, st, dev(NOISE), P))
    torch.cuda.synchronize()
    filt.OnDestroy()


@pytest.mark.parametrize("shape", [(66, 19, 132, 38), (97, 61, 131, 83)], ids=["exact2x", "generic"])
def test_easu_h_stages_last_pass(fsr, port, shape):
    """fsr1_upscale_ex with use_rcas = 0: SRTM at EASU-H's loads, grain + TEPD at its stores, RGBA16F -> RGBA8."""
    iw, ih, ow, oh = shape
    st = SETS["B"]
    x = source("f16", iw, ih, st, 5)
    out = FMT["rgba8"].empty(oh, ow)
    assert plan(fsr, iw, ih, ow, oh, "f16", "rgba8", 0, 0) == 2
    upscale(fsr, dev(x), out, iw, ih, ow, oh, False, False, st)
    con = port.FsrEasuCon(iw, ih, iw, ih, ow, oh)
    check("rgba8", out, oracle(port, x.astype(np.float32), st, easu=(ow, oh, con)), "easu H + stages")


@pytest.mark.parametrize("fused", [False, "auto"], ids=["two-pass", "auto"])
@pytest.mark.parametrize("sset", ["A", "B"])
@pytest.mark.parametrize("fmt", ["rgba8", "f16"])
def test_chain_h_stages(fsr, port, fmt, sset, fused):
    iw, ih, ow, oh = 66, 19, 132, 38
    st = SETS[sset]
    x = source(fmt, iw, ih, st, 9)
    out = FMT[fmt].empty(oh, ow)
    assert plan(fsr, iw, ih, ow, oh, fmt, fmt, 1, 2) == 0  # packed fp16 + stages: `auto` always plans the two dispatches
    upscale(fsr, FMT[fmt].up(x), out, iw, ih, ow, oh, True, fused, st)
    con, rcon = port.FsrEasuCon(iw, ih, iw, ih, ow, oh), port.FsrRcasCon(0.25)
    check(fmt, out, oracle(port, FMT[fmt].dec(x), st, fmt, (ow, oh, con), rcon), "chain H %s set %s" % (fmt, sset))


def test_chain_h_stages_pipeline_batch(fsr, port):
    """Two frames in tensors whose rows are longer than the image, through a two-stream pipeline."""
    iw, ih, ow, oh, n, st = 66, 19, 132, 38, 2, SETS["B"]
    x = source("f16", iw, ih, st, 13, n)
    src, dst = F16.empty(n, ih, iw + 3)[:, :, :iw], F16.empty(n, oh, ow + 5)[:, :, :ow]
    src.copy_(dev(x))
    pipe = fsr.Pipeline(2)
    pipe.upscale(src, dst, sharpness=0.25, fused=2, flags=H_STAGES, stages=stages_of(fsr, st, dev(NOISE), P))
    pipe.synchronize()
    pipe.close()
    con, rcon = port.FsrEasuCon(iw, ih, iw, ih, ow, oh), port.FsrRcasCon(0.25)
    for k in range(n):
        check("f16", dst[k].contiguous(), oracle(port, x[k].astype(np.float32), st, "f16", (ow, oh, con), rcon), "pipeline frame %d" % k)


@pytest.mark.parametrize("fin,fout,sset", [("rgba8", "rgba8", "B"), ("f16", "rgb10a2", "C"), ("rgb10a2", "f16", "A")], ids=lambda v: str(v))
def test_color_pass_h_formats(fsr, port, fin, fout, sset):
    """131 x 9 (one pixel short of 33 lanes' four); the same-format case runs in place."""
    st, (w, h) = SETS[sset], (131, 9)
    x = source(fin, w, h, st, 17)
    src = FMT[fin].up(x)
    out = src if fin == fout else FMT[fout].empty(h, w)
    fsr.color(src, out, stages_of(fsr, st, dev(NOISE), P), flags=fsr.FLAG_MATH_PACKED_FP16)
    check(fout, out, oracle(port, FMT[fin].dec(x), st), "color H %s -> %s" % (fin, fout))


def test_refusals_that_stay(fsr):
    H, cs = H_STAGES, fsr.ColorStages(1 | 4)
    a, b, f32 = F16.empty(8, 8), F16.empty(8, 8), torch.zeros(8, 8, 4, dtype=torch.float32, device="cuda")
    with pytest.raises(fsr.Fsr1Error, match="error -2"):
        fsr.easu_rcas_fused(a, F16.empty(16, 16), flags=H, stages=cs)
    with pytest.raises(fsr.Fsr1Error, match="error -2"):
        fsr.rcas(f32, torch.zeros_like(f32), flags=H, stages=cs)
    with pytest.raises(fsr.Fsr1Error, match="error -2"):
        fsr.rcas_band(a, b, flags=H)
    assert plan(fsr, 66, 19, 132, 38, "f16", "f16", 1, 1) == -2
    with pytest.raises(fsr.Fsr1Error, match="error -2"):  # and without the opt-in bit packed fp16 with stages stays refused
        fsr.rcas(a, b, flags=fsr.FLAG_MATH_PACKED_FP16, stages=cs)
