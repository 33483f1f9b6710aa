#!/usr/bin/env python3
"""Packed 3-channel RGB against RGBA of the same element type at 1920x1080 -> 3840x2160, default arithmetic, one frame per call:
FORMAT_RGB16F against RGBA16F, or (--dtype u8) FORMAT_RGB8_UNORM against RGBA8_UNORM.

  python tools/rgb_bench.py --out profiles/rgb_1080p_to_4k.json
  python tools/rgb_bench.py --dtype u8 --out profiles/rgb_u8_1080p_to_4k.json

The protocol is tools/planar_bench.py's: every configuration is timed between two events on the current stream over `--calls`
back-to-back calls, seven windows per configuration with the configurations alternating, each walking a ring of buffer sets larger
than the 256 MB Infinity Cache.  Needs a GPU: there is no fallback."""
import argparse
import importlib
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools.planar_bench import smi  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--calls", type=int, default=300)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--ring", type=int, default=8)
    ap.add_argument("--dtype", choices=["f16", "u8"], default="f16")
    args = ap.parse_args()
    import torch
    fsr = importlib.import_module("fidelityfx-fsr_amd")
    fsr.load()
    if not torch.cuda.is_available():
        raise SystemExit("rgb_bench needs a GPU")
    iw, ih, ow, oh = 1920, 1080, 3840, 2160
    con, rcon = fsr.FsrEasuCon(iw, ih, iw, ih, ow, oh), fsr.FsrRcasCon(0.25)
    R = fsr.Rgb
    u8 = args.dtype == "u8"
    tdt, inter = (torch.uint8, "rgba8") if u8 else (torch.float16, "rgba16f")
    rgba = torch.from_numpy(fsr.frames.synthetic_frame(iw, ih, k=0)).cuda()
    if u8:  # the store rule of RGBA8_UNORM (include/fsr1_hip.h), alpha at its maximum
        rgba = (rgba.float().clamp(0, 1) * 255 + 0.5).to(torch.uint8)
        rgba[..., 3] = 255
    hwc = rgba[..., :3].contiguous()

    def ring(make):
        return [make() for _ in range(args.ring)]

    z = lambda *s: torch.zeros(*s, dtype=tdt, device="cuda")  # noqa: E731
    r_in, r_mid, r_out = ring(lambda: hwc.clone()), ring(lambda: z(oh, ow, 3)), ring(lambda: z(oh, ow, 3))
    i_in, i_mid, i_out = ring(lambda: rgba.clone()), ring(lambda: z(oh, ow, 4)), ring(lambda: z(oh, ow, 4))
    for k in range(args.ring):  # real intermediaries for the RCAS-only configurations
        fsr.easu(R(r_in[k]), R(r_mid[k]), con=con)
        fsr.easu(i_in[k], i_mid[k], con=con)
    ones = torch.full((ih, iw, 1), 255 if u8 else 1, dtype=tdt, device="cuda")

    def pad_slice(k):
        """What a caller of the RGBA ABI does for an (H,W,3) tensor today: pad to four channels, the RGBA chain, slice to three."""
        fsr.easu(torch.cat([r_in[k], ones], -1), i_mid[k], con=con)
        fsr.rcas(i_mid[k], i_out[k], con=rcon)
        return i_out[k][..., :3].contiguous()

    def chain_rgb(k):
        fsr.easu(R(r_in[k]), R(r_mid[k]), con=con)
        fsr.rcas(R(r_mid[k]), R(r_out[k]), con=rcon)

    def chain_rgba(k):
        fsr.easu(i_in[k], i_mid[k], con=con)
        fsr.rcas(i_mid[k], i_out[k], con=rcon)

    configs = {
        "rcas_rgb": lambda k: fsr.rcas(R(r_mid[k]), R(r_out[k]), con=rcon),
        "rcas_%s" % inter: lambda k: fsr.rcas(i_mid[k], i_out[k], con=rcon),
        "easu_rgb": lambda k: fsr.easu(R(r_in[k]), R(r_mid[k]), con=con),
        "easu_%s" % inter: lambda k: fsr.easu(i_in[k], i_mid[k], con=con),
        "chain_rgb": chain_rgb,
        "chain_%s" % inter: chain_rgba,
        "chain_%s_pad_slice" % inter: pad_slice,
    }
    # the 3-channel chain and the padded RGBA chain compute the same image
    chain_rgb(0)
    same = bool(torch.equal(r_out[0], pad_slice(0)))
    for fn in configs.values():  # warm every kernel on every buffer set
        for k in range(args.ring):
            fn(k)
    torch.cuda.synchronize()
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
        "what": "packed 3-channel RGB %s against %s, %dx%d -> %dx%d, default arithmetic, one frame per call; %d calls per window between two "
                "events on one stream, %d windows per configuration, the configurations alternating, each on a ring of %d buffer sets"
                % ((("uint8", "RGBA8_UNORM") if u8 else ("fp16", "RGBA16F")) + (iw, ih, ow, oh, args.calls, args.windows, args.ring)),
        "device": torch.cuda.get_device_name(0),
        "clocks_and_power_after_the_run": smi(),
        "rgb_chain_equals_pad_slice_chain": same,
        "us_per_call": {k: {"median": round(statistics.median(v), 2), "min": round(min(v), 2), "max": round(max(v), 2)} for k, v in times.items()},
        "build_id": fsr._lib.build_id(),
    }
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc["us_per_call"], indent=1))
    print("rgb == pad / slice:", same)


if __name__ == "__main__":
    main()
