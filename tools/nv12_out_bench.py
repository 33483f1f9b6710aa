#!/usr/bin/env python3
"""RCAS with the NV12 store at 3840x2160, and the NV12 -> NV12 chain 1920x1080 -> 3840x2160, default arithmetic, one frame per call
(tools/nv12_bench.py's protocol):

  rcas_nv12_from_{f16,u8}   RCAS from fp16 / uint8 planes straight into an NV12 surface (fsr1_rcas_dispatch_ycbcr)
  rcas_planar_{f16,u8}      planar RCAS of the same planes in the same run: what the NV12 store is compared with
  transcode_{f16,u8}        fsr1_transcode_ycbcr: NV12 -> EASU -> fp16 / uint8 planes -> RCAS -> NV12
  transcode_detour_u8       what such a caller paid before: fsr1_upscale_ycbcr into planar uint8, then a torch RGB -> NV12 conversion
                            with box chroma over the 4K planes

  python tools/nv12_out_bench.py --out profiles/nv12_out_1080p_to_4k.json

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
        raise SystemExit("nv12_out_bench needs a GPU")
    iw, ih, ow, oh = 1920, 1080, 3840, 2160
    P, N, yc, conv = fsr.Planar, fsr.Nv12, fsr.YCbCr.bt709(), fsr.RgbToYCbCr.bt709()
    m, bias = torch.from_numpy(yc.m).cuda(), torch.from_numpy(yc.bias).cuda()
    fm, fbias = torch.from_numpy(conv.m).cuda(), torch.from_numpy(conv.bias).cuda()

    def to_nv12(planes_u8, surf):
        """The detour's conversion in torch: (3, H, W) uint8 planes -> the (rows, W) NV12 surface, chroma = the 2 x 2 box of the RGB."""
        rgb = planes_u8.float().div_(255)
        surf[:oh] = (torch.einsum("kc,chw->khw", fm[:1], rgb)[0] + fbias[0]).clamp_(0, 255).add_(0.5).to(torch.uint8)
        box = rgb.view(3, oh // 2, 2, ow // 2, 2).mean(dim=(2, 4))
        c = (torch.einsum("kc,chw->hwk", fm[1:], box) + fbias[1:]).clamp_(0, 255).add_(0.5).to(torch.uint8)
        surf[oh:] = c.reshape(oh // 2, ow)
        return surf

    # frame 0 of the synthetic sequence as an NV12 surface (tools/nv12_bench.py), and as 4K planes for the RCAS-only configurations
    rgb = torch.from_numpy(fsr.frames.synthetic_frame(iw, ih, k=0)).cuda()[..., :3].float()
    ycc = ((rgb - bias) @ torch.linalg.inv(m).T).round_().clamp_(0, 255)
    chroma = ycc[..., 1:].view(ih // 2, 2, iw // 2, 2, 2).mean(dim=(1, 3)).round_()
    nv12 = torch.cat([ycc[..., 0], chroma.reshape(ih // 2, iw)], 0).to(torch.uint8)
    big = torch.from_numpy(fsr.frames.synthetic_frame(ow, oh, k=0)).cuda()[..., :3].float().permute(2, 0, 1).contiguous()

    def ring(make):
        return [make() for _ in range(args.ring)]

    z = lambda dt: torch.zeros(3, oh, ow, dtype=dt, device="cuda")  # noqa: E731
    surf = lambda: torch.zeros(oh * 3 // 2, ow, dtype=torch.uint8, device="cuda")  # noqa: E731
    n_in = ring(nv12.clone)
    i16, i8 = ring(lambda: big.half()), ring(lambda: (big * 255 + 0.5).to(torch.uint8))
    o16, o8, on = ring(lambda: z(torch.float16)), ring(lambda: z(torch.uint8)), ring(surf)
    m16, m8 = ring(lambda: z(torch.float16)), ring(lambda: z(torch.uint8))

    def detour(k):
        fsr.upscale_ycbcr(N(n_in[k]), P(m8[k]), P(o8[k]), yc, sharpness=0.25)
        return to_nv12(o8[k], on[k])

    configs = {
        "rcas_nv12_from_f16": lambda k: fsr.rcas(P(i16[k]), N(on[k]), sharpness=0.25, ycbcr=conv),
        "rcas_nv12_from_u8": lambda k: fsr.rcas(P(i8[k]), N(on[k]), sharpness=0.25, ycbcr=conv),
        "rcas_planar_f16": lambda k: fsr.rcas(P(i16[k]), P(o16[k]), sharpness=0.25),
        "rcas_planar_u8": lambda k: fsr.rcas(P(i8[k]), P(o8[k]), sharpness=0.25),
        "transcode_f16": lambda k: fsr.transcode_ycbcr(N(n_in[k]), P(m16[k]), N(on[k]), yc, conv, sharpness=0.25),
        "transcode_u8": lambda k: fsr.transcode_ycbcr(N(n_in[k]), P(m8[k]), N(on[k]), yc, conv, sharpness=0.25),
        "transcode_detour_u8": detour,
    }
    for fn in configs.values():  # warm every kernel on every buffer set
        for k in range(args.ring):
            fn(k)
    torch.cuda.synchronize()
    # the two chains give the same surface up to the detour's 8-bit RGB rounding in front of its conversion
    native = configs["transcode_u8"](0).t.clone()
    chain_gap = float((native.float() - detour(0).float()).abs().mean())
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
        "what": "RCAS with the NV12 store against planar RCAS at %dx%d, and the NV12 -> NV12 chain %dx%d -> %dx%d against the torch-conversion "
                "detour, default arithmetic, BT.709 limited range, siting LEFT in / CENTER out, one frame per call; %d calls per window between two "
                "events on one stream, %d windows per configuration, the configurations alternating, a ring of %d buffer sets"
                % (ow, oh, iw, ih, ow, oh, args.calls, args.windows, args.ring),
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
    print("mean |native - detour| in codes =", chain_gap)


if __name__ == "__main__":
    main()
