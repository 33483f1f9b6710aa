#!/usr/bin/env python3
"""P010 against NV12 through EASU and RCAS, 1920x1080 -> 3840x2160, default arithmetic, BT.2020 limited range, siting LEFT in / CENTER
out, one frame per call (tools/nv12_bench.py's protocol), everything in one run:

  easu_{p010,nv12}        EASU of the surface into fp16 planes (fsr1_easu_dispatch_ycbcr)
  rcas_{p010,nv12}        RCAS from fp16 planes straight into the surface (fsr1_rcas_dispatch_ycbcr)
  transcode_{p010,nv12}   fsr1_transcode_ycbcr through fp16 planes, surface to surface of the same format
  transcode_detour_p010   what a P010 caller paid before: torch P010 -> fp16 planes at 1080p, the planar chain, torch planes -> P010 at 4K

  python tools/p010_bench.py --out profiles/p010_1080p_to_4k.json

Every configuration is timed between two events on the current stream over `--calls` back-to-back calls, seven windows per
configuration with the configurations alternating, over a ring of buffer sets larger than the 256 MB Infinity Cache.  Needs a GPU:
there is no fallback."""
import argparse
import importlib
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--calls", type=int, default=300)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--ring", type=int, default=8)
    args = ap.parse_args()
    import torch
    from planar_bench import smi
    fsr = importlib.import_module("fidelityfx-fsr_amd")
    fsr.load()
    if not torch.cuda.is_available():
        raise SystemExit("p010_bench needs a GPU")
    iw, ih, ow, oh = 1920, 1080, 3840, 2160
    P = fsr.Planar
    rgb = torch.from_numpy(fsr.frames.synthetic_frame(iw, ih, k=0)).cuda()[..., :3].float()
    big = torch.from_numpy(fsr.frames.synthetic_frame(ow, oh, k=0)).cuda()[..., :3].float().permute(2, 0, 1).contiguous()

    def surface_of(bits):
        """Frame 0 of the synthetic sequence as the (rows, W) surface of that depth: uint8 codes, or int16 words with the code on top."""
        yc = fsr.YCbCr.bt2020(bits=bits)
        m, bias = torch.from_numpy(yc.m).cuda(), torch.from_numpy(yc.bias).cuda()
        ycc = ((rgb - bias) @ torch.linalg.inv(m).T).round_().clamp_(0, 2 ** bits - 1)
        chroma = ycc[..., 1:].view(ih // 2, 2, iw // 2, 2, 2).mean(dim=(1, 3)).round_()
        codes = torch.cat([ycc[..., 0], chroma.reshape(ih // 2, iw)], 0).to(torch.int32)
        return codes.to(torch.uint8) if bits == 8 else (codes << (16 - bits)).to(torch.int16)

    yc10, conv10, yc8, conv8 = fsr.YCbCr.bt2020(bits=10), fsr.RgbToYCbCr.bt2020(bits=10), fsr.YCbCr.bt2020(), fsr.RgbToYCbCr.bt2020()
    m10, b10 = torch.from_numpy(yc10.m).cuda(), torch.from_numpy(yc10.bias).cuda()
    f10, fb10 = torch.from_numpy(conv10.m).cuda(), torch.from_numpy(conv10.bias).cuda()

    def from_p010(surf, planes):
        """The detour's way in, in torch: words -> codes -> replicated chroma -> (3, H, W) fp16 planes."""
        codes = (surf.to(torch.int32) & 0xFFFF) >> 6
        c = codes[ih:].view(ih // 2, iw // 2, 2).repeat_interleave(2, 0).repeat_interleave(2, 1)
        ycc = torch.cat([codes[:ih, :, None], c], -1).float()
        planes.copy_((torch.einsum("kc,hwc->khw", m10, ycc) + b10[:, None, None]).clamp_(0, 1))
        return planes

    def to_p010(planes, surf):
        """... and out: (3, H, W) fp16 planes -> words, chroma = the 2 x 2 box of the RGB."""
        p = planes.float()
        y = (torch.einsum("c,chw->hw", f10[0], p) + fb10[0]).clamp_(0, 1023).add_(0.5).to(torch.int32)
        box = p.view(3, oh // 2, 2, ow // 2, 2).mean(dim=(2, 4))
        c = (torch.einsum("kc,chw->hwk", f10[1:], box) + fb10[1:]).clamp_(0, 1023).add_(0.5).to(torch.int32)
        surf.copy_((torch.cat([y, c.reshape(oh // 2, ow)], 0) << 6).to(torch.int16))
        return surf

    def ring(make):
        return [make() for _ in range(args.ring)]

    z16 = lambda h, w: torch.zeros(3, h, w, dtype=torch.float16, device="cuda")  # noqa: E731
    p_in, n_in = ring(surface_of(10).clone), ring(surface_of(8).clone)
    p_out = ring(lambda: torch.zeros(oh * 3 // 2, ow, dtype=torch.int16, device="cuda"))
    n_out = ring(lambda: torch.zeros(oh * 3 // 2, ow, dtype=torch.uint8, device="cuda"))
    i16, mid, small, o16 = ring(lambda: big.half()), ring(lambda: z16(oh, ow)), ring(lambda: z16(ih, iw)), ring(lambda: z16(oh, ow))

    def detour(k):
        fsr.easu(P(from_p010(p_in[k], small[k])), P(mid[k]))
        fsr.rcas(P(mid[k]), P(o16[k]), sharpness=0.25)
        return to_p010(o16[k], p_out[k])

    configs = {
        "easu_p010": lambda k: fsr.easu(fsr.P010(p_in[k]), P(mid[k]), ycbcr=yc10),
        "easu_nv12": lambda k: fsr.easu(fsr.Nv12(n_in[k]), P(mid[k]), ycbcr=yc8),
        "rcas_p010": lambda k: fsr.rcas(P(i16[k]), fsr.P010(p_out[k]), sharpness=0.25, ycbcr=conv10),
        "rcas_nv12": lambda k: fsr.rcas(P(i16[k]), fsr.Nv12(n_out[k]), sharpness=0.25, ycbcr=conv8),
        "transcode_p010": lambda k: fsr.transcode_ycbcr(fsr.P010(p_in[k]), P(mid[k]), fsr.P010(p_out[k]), yc10, conv10, sharpness=0.25),
        "transcode_nv12": lambda k: fsr.transcode_ycbcr(fsr.Nv12(n_in[k]), P(mid[k]), fsr.Nv12(n_out[k]), yc8, conv8, sharpness=0.25),
        "transcode_detour_p010": detour,
    }
    for fn in configs.values():  # warm every kernel on every buffer set
        for k in range(args.ring):
            fn(k)
    torch.cuda.synchronize()
    # the two chains give the same surface up to the detour's replicated chroma on the way in and its fp16 planes on the way out
    native = (configs["transcode_p010"](0).t.to(torch.int32) & 0xFFFF) >> 6
    chain_gap = float((native - ((detour(0).to(torch.int32) & 0xFFFF) >> 6)).abs().float().mean())
    times = {name: [] for name in configs}
    for _ in range(args.windows):
        for name, fn in configs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for c in range(args.calls):
                fn(c % args.ring)
            e1.record()
            e1.synchronize()
            times[name].append(e0.elapsed_time(e1) * 1000.0 / args.calls)
    doc = {
        "what": "P010 against NV12: EASU into fp16 planes, RCAS from fp16 planes into the surface, and the surface-to-surface chain %dx%d -> %dx%d "
                "against the torch-conversion detour of a P010 caller; default arithmetic, BT.2020 limited range, siting LEFT in / CENTER out, one "
                "frame per call; %d calls per window between two events on one stream, %d windows per configuration, the configurations "
                "alternating, a ring of %d buffer sets" % (iw, ih, ow, oh, args.calls, args.windows, args.ring),
        "device": torch.cuda.get_device_name(0),
        "clocks_and_power_after_the_run": smi(),
        "mean_abs_code_difference_of_the_two_chains": chain_gap,
        "us_per_call": {k: {"median": round(statistics.median(v), 2), "min": round(min(v), 2), "max": round(max(v), 2)} for k, v in times.items()},
        "build_id": fsr._lib.build_id(),
    }
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc["us_per_call"], indent=1))
    print("mean |native - detour| in 10-bit codes =", chain_gap)


if __name__ == "__main__":
    main()
