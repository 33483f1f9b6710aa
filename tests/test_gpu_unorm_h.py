"""Class H (packed binary16, FsrEasuH / FsrRcasH) on 32 bpp UNORM storage — the reference's shipping combination.
    load  = code / (2^n - 1) correctly rounded to binary32, then RTNE to binary16 (what the oracle's H entry points do to their input)
    store = the binary16 result widened, then (uint) fma(clamp(x,0,1), 2^n - 1, 0.5) (NaN -> 0)
Class H is bit-identical to the CPU-evaluated reference, so every assertion is "every code equal"."""
import importlib

import numpy as np
import pytest

from test_gpu_unorm import decode, encode, pack10, rgba8_frame, unpack10

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
frames = importlib.import_module("fidelityfx-fsr_amd.frames")


class Rgba8:
    amax = 255
    dec = staticmethod(lambda c: decode(c, 255))
    enc = staticmethod(lambda x: encode(x, 255).astype(np.uint8))
    frame = staticmethod(rgba8_frame)
    up = staticmethod(lambda c: torch.from_numpy(np.ascontiguousarray(c)).cuda())
    host = staticmethod(lambda t: t.cpu().numpy())
    empty = staticmethod(lambda *lead: torch.zeros(*lead, 4, dtype=torch.uint8, device="cuda"))

    @staticmethod
    def with_alpha(codes, a):
        out = codes.copy()
        out[..., 3] = a
        return out


class Rgb10a2:
    amax = 3
    dec, enc = staticmethod(unpack10), staticmethod(pack10)
    up = staticmethod(lambda w: torch.from_numpy(np.ascontiguousarray(w).view(np.int32)).cuda())
    host = staticmethod(lambda t: t.cpu().numpy().view(np.uint32))
    empty = staticmethod(lambda *lead: torch.zeros(*lead, dtype=torch.int32, device="cuda"))

    @staticmethod
    def frame(w, h, k):
        img = frames.synthetic_frame(w, h, k=k, dtype=np.float32)
        img[..., 3] = (np.arange(w)[None, :] % 4) / 3.0  # the alpha ramp of test_rgb10a2_pipeline
        return pack10(img)

    @staticmethod
    def with_alpha(words, a):
        return (words & np.uint32(0x3FFFFFFF)) | (a.astype(np.uint32) << 30)


FORMATS = {"rgba8": Rgba8, "rgb10a2": Rgb10a2}
# smaller than a tile and than a lane's four pixels | generic ratio, ragged, crosses the 64 x 16 EASU tiles | exact 2x (S2 EASU-H, the
# exact-2x fused H) | RCAS strips: the wave seam at column 256, the workgroup seam at 512, width mod 4 = 3, three 8-row strips
SHAPES = [(5, 3, 17, 9), (97, 61, 131, 83), (66, 19, 132, 38), (130, 9, 515, 17)]
ORACLE_DENOISE_ALPHA = 3


def same(got, want, what):
    d = got != want
    assert not d.any(), "%s: %d of %d codes differ" % (what, int(d.sum()), d.size)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d_to_%dx%d" % s)
@pytest.mark.parametrize("fmt", sorted(FORMATS))
def test_unorm_h_pipeline(fsr, port, fmt, shape):
    F = FORMATS[fmt]
    iw, ih, ow, oh = shape
    H = fsr.FLAG_MATH_PACKED_FP16
    opts = fsr.FLAG_RCAS_DENOISE | fsr.FLAG_RCAS_PASSTHROUGH_ALPHA
    codes = F.frame(iw, ih, 5)
    con, rcon = port.FsrEasuCon(iw, ih, iw, ih, ow, oh), port.FsrRcasCon(0.25)
    src, mid, out, out_o, fus, fus_o = F.up(codes), F.empty(oh, ow), F.empty(oh, ow), F.empty(oh, ow), F.empty(oh, ow), F.empty(oh, ow)
    fsr.easu(src, mid, con=con, flags=H)
    fsr.rcas(mid, out, con=rcon, flags=H)
    fsr.rcas(mid, out_o, con=rcon, flags=H | opts)
    fsr.easu_rcas_fused(src, fus, easu_con=con, rcas_con=rcon, flags=H)
    fsr.easu_rcas_fused(src, fus_o, easu_con=con, rcas_con=rcon, flags=H | opts)
    torch.cuda.synchronize()
    got_mid = F.host(mid)
    same(got_mid, F.enc(port.easu_h(F.dec(codes), ow, oh, con)), "easu H " + fmt)
    # stage-wise: RCAS against the oracle run on the GPU's own intermediary
    same(F.host(out), F.enc(port.rcas_h(F.dec(got_mid), rcon, 0)), "rcas H " + fmt)
    # ... and with denoise + alpha pass-through on that intermediary given an alpha ramp (EASU's own alpha is 1 everywhere)
    ramp = F.with_alpha(got_mid, (np.arange(ow)[None, :] + np.arange(oh)[:, None]) % (F.amax + 1))
    out_r = F.empty(oh, ow)
    fsr.rcas(F.up(ramp), out_r, con=rcon, flags=H | opts)
    same(F.host(out_r), F.enc(port.rcas_h(F.dec(ramp), rcon, ORACLE_DENOISE_ALPHA)), "rcas H denoise + alpha " + fmt)
    # the fused launch = the two dispatches with an intermediary of the output's format
    same(F.host(fus), F.host(out), "fused H " + fmt)
    same(F.host(fus_o), F.host(out_o), "fused H denoise + alpha " + fmt)
    # the reference's host glue with its default permutation (packed fp16), as two dispatches, one launch and `auto`
    for fused in (False, True, "auto"):
        filt = fsr.FSR_Filter()
        filt.OnCreate(slowFallback=False, fused=fused)
        dst = F.empty(oh, ow)
        filt.OnCreateWindowSizeDependentResources(src, dst, ow, oh)
        filt.Upscale(ow, oh, fsr.State(iw, ih, bUseRcas=True, rcasAttenuation=0.25))
        torch.cuda.synchronize()
        same(F.host(dst), F.host(out), "FSR_Filter fused=%s %s" % (fused, fmt))
        filt.OnDestroy()


@pytest.mark.parametrize("fmt", sorted(FORMATS))
def test_unorm_h_batch_with_padded_pitch(fsr, port, fmt):
    """Three frames in tensors whose rows are longer than the image: every pass, the fused launch and the stream pipeline."""
    F = FORMATS[fmt]
    iw, ih, ow, oh, n = 37, 11, 74, 22, 3
    H = fsr.FLAG_MATH_PACKED_FP16
    codes = np.stack([F.frame(iw, ih, k) for k in range(n)])
    con, rcon = port.FsrEasuCon(iw, ih, iw, ih, ow, oh), port.FsrRcasCon(0.25)
    src = F.empty(n, ih, iw + 3)[:, :, :iw]
    src.copy_(F.up(codes))
    mid, out, fus, pip = (F.empty(n, oh, ow + 5)[:, :, :ow] for _ in range(4))
    fsr.easu(src, mid, con=con, flags=H)
    fsr.rcas(mid, out, con=rcon, flags=H)
    fsr.easu_rcas_fused(src, fus, easu_con=con, rcas_con=rcon, flags=H)
    pipe = fsr.Pipeline(2)
    pipe.upscale(src, pip, sharpness=0.25, fused=0, flags=H)
    pipe.synchronize()
    pipe.close()
    torch.cuda.synchronize()
    got_mid = F.host(mid.contiguous())
    for k in range(n):
        same(got_mid[k], F.enc(port.easu_h(F.dec(codes[k]), ow, oh, con)), "easu H frame %d" % k)
        same(F.host(out.contiguous())[k], F.enc(port.rcas_h(F.dec(got_mid[k]), rcon, 0)), "rcas H frame %d" % k)
    same(F.host(fus.contiguous()), F.host(out.contiguous()), "fused H batch")
    same(F.host(pip.contiguous()), F.host(out.contiguous()), "pipeline H batch")
