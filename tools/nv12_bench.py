#!/usr/bin/env python3
"""A decoder's NV12 frame at 1920x1080 -> 3840x2160, default arithmetic, one frame per call (tools/rgb_bench.py's protocol):

  easu_nv12_{f16,f32,u8}   the NV12 EASU (conversion inside the footprint staging) into each planar output type
  easu_planar_u8           planar uint8 EASU on the same frame already converted to RGB: what the NV12 kernel is compared with
  chain_nv12_f16           fsr1_upscale_ycbcr: NV12 -> EASU -> planar fp16 RCAS, the tensor a model takes
  chain_detour_f16         what such a caller paid before: a torch NV12 -> RGB uint8 conversion (chroma replicated, the cheapest a
                           caller writes), the planar uint8 chain, then .to(float16) / 255

  python tools/nv12_bench.py --out profiles/nv12_1080p_to_4k.json

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
        raise SystemExit("nv12_bench needs a GPU")
    iw, ih, ow, oh = 1920, 1080, 3840, 2160
    con = fsr.FsrEasuCon(iw, ih, iw, ih, ow, oh)
    P, yc = fsr.Planar, fsr.YCbCr.bt709()
    m, bias = torch.from_numpy(yc.m).cuda(), torch.from_numpy(yc.bias).cuda()

    def to_rgb_u8(surf):
        """The detour's conversion in torch: (rows, W) NV12 surface -> (3, H, W) uint8 planes, chroma replicated."""
        c = surf[ih:].view(ih // 2, iw // 2, 2).float().repeat_interleave(2, 0).repeat_interleave(2, 1)
        rgb = (torch.cat([surf[:ih].float().unsqueeze(-1), c], -1) @ m.T + bias).clamp_(0, 1)
        return (rgb * 255 + 0.5).to(torch.uint8).permute(2, 0, 1).contiguous()

    # frame 0 of the synthetic sequence as an NV12 surface: forward transform on the GPU, chroma = the mean of each 2 x 2 block
    rgb = torch.from_numpy(fsr.frames.synthetic_frame(iw, ih, k=0)).cuda()[..., :3].float()
    ycc = ((rgb - bias) @ torch.linalg.inv(m).T).round_().clamp_(0, 255)
    chroma = ycc[..., 1:].view(ih // 2, 2, iw // 2, 2, 2).mean(dim=(1, 3)).round_()
    nv12 = torch.cat([ycc[..., 0], chroma.reshape(ih // 2, iw)], 0).to(torch.uint8)

    def ring(make):
        return [make() for _ in range(args.ring)]

    z = lambda dt: torch.zeros(3, oh, ow, dtype=dt, device="cuda")  # noqa: E731
    n_in, u_in = ring(nv12.clone), ring(lambda: to_rgb_u8(nv12))
    o16, o32, o8 = ring(lambda: z(torch.float16)), ring(lambda: z(torch.float32)), ring(lambda: z(torch.uint8))
    m16, m8 = ring(lambda: z(torch.float16)), ring(lambda: z(torch.uint8))

    def detour(k):
        u = to_rgb_u8(n_in[k])
        fsr.easu(P(u), P(m8[k]), con=con)
        fsr.rcas(P(m8[k]), P(o8[k]), sharpness=0.25)
        return o8[k].to(torch.float16) / 255

    configs = {
        "easu_nv12_f16": lambda k: fsr.easu(fsr.Nv12(n_in[k]), P(o16[k]), con=con, ycbcr=yc),
        "easu_nv12_f32": lambda k: fsr.easu(fsr.Nv12(n_in[k]), P(o32[k]), con=con, ycbcr=yc),
        "easu_nv12_u8": lambda k: fsr.easu(fsr.Nv12(n_in[k]), P(o8[k]), con=con, ycbcr=yc),
        "easu_planar_u8": lambda k: fsr.easu(P(u_in[k]), P(o8[k]), con=con),
        "chain_nv12_f16": lambda k: fsr.upscale_ycbcr(fsr.Nv12(n_in[k]), P(m16[k]), P(o16[k]), yc, sharpness=0.25),
        "chain_detour_f16": detour,
    }
    for fn in configs.values():  # warm every kernel on every buffer set
        for k in range(args.ring):
            fn(k)
    torch.cuda.synchronize()
    # the two chains give the same tensor up to the detour's two 8-bit roundings and its replicated chroma
    chain_gap = float((configs["chain_nv12_f16"](0).t.float() - detour(0).float()).abs().mean())
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
        "what": "NV12 EASU against planar uint8 EASU, and the NV12 -> fp16 chain against the torch-conversion detour, %dx%d -> %dx%d, default "
                "arithmetic, BT.709 limited range, siting LEFT, one frame per call; %d calls per window between two events on one stream, %d windows "
                "per configuration, the configurations alternating, a ring of %d buffer sets" % (iw, ih, ow, oh, args.calls, args.windows, args.ring),
        "device": torch.cuda.get_device_name(0),
        "clocks_and_power_after_the_run": smi(),
        "mean_abs_difference_of_the_two_chains": chain_gap,
        "us_per_call": {k: {"median": round(statistics.median(v), 2), "min": round(min(v), 2), "max": round(max(v), 2)} for k, v in times.items()},
        "build_id": fsr._lib.build_id(),
    }
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc["us_per_call"], indent=1))
    print("mean |native - detour| =", chain_gap)


if __name__ == "__main__":
    main()
