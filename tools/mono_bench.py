#!/usr/bin/env python3
"""Single-channel images against RGBA of the same element type at 1920x1080 -> 3840x2160, default arithmetic, one frame per call:
FORMAT_R16F against RGBA16F, or (--dtype u8) FORMAT_R8_UNORM against RGBA8_UNORM, and the detour a caller of the RGBA ABI pays for a luma
plane today (replicate to RGBA -> RGBA chain -> take channel 0).

  python tools/mono_bench.py --out profiles/mono_1080p_to_4k.json
  python tools/mono_bench.py --dtype u8 --out profiles/mono_u8_1080p_to_4k.json

The protocol is tools/rgb_bench.py's: every configuration is timed between two events on the current stream over `--calls` back-to-back
calls, seven windows per configuration with the configurations alternating, each walking a ring of buffer sets.  Other launch shapes
of the single-channel RCAS kernel (columns per lane x rows per strip) are tuning builds (tools/build_variant.sh with a patch of
rcas_mono_geometry), timed with FSR1_HIP_LIB=variants/... and --only rcas.  Needs a GPU: there is no fallback."""
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
    ap.add_argument("--only", default="", help="time only the configurations whose name starts with this (a tuning build of another launch shape: rcas)")
    args = ap.parse_args()
    import torch
    fsr = importlib.import_module("fidelityfx-fsr_amd")
    fsr.load()
    if not torch.cuda.is_available():
        raise SystemExit("mono_bench needs a GPU")
    iw, ih, ow, oh = 1920, 1080, 3840, 2160
    con, rcon = fsr.FsrEasuCon(iw, ih, iw, ih, ow, oh), fsr.FsrRcasCon(0.25)
    M = fsr.Mono
    u8 = args.dtype == "u8"
    tdt, inter = (torch.uint8, "rgba8") if u8 else (torch.float16, "rgba16f")
    rgba = torch.from_numpy(fsr.frames.synthetic_frame(iw, ih, k=0)).cuda()
    if u8:  # the store rule of RGBA8_UNORM (include/fsr1_hip.h)
        rgba = (rgba.float().clamp(0, 1) * 255 + 0.5).to(torch.uint8)
    luma = rgba[..., 1].contiguous()
    rgba = luma[..., None].expand(ih, iw, 4).contiguous()  # (L, L, L, 1): the twin's input
    rgba[..., 3] = 255 if u8 else 1

    def ring(make):
        return [make() for _ in range(args.ring)]

    z = lambda *s: torch.zeros(*s, dtype=tdt, device="cuda")  # noqa: E731
    m_in, m_mid, m_out = ring(lambda: luma.clone()), ring(lambda: z(oh, ow)), ring(lambda: z(oh, ow))
    i_in, i_mid, i_out = ring(lambda: rgba.clone()), ring(lambda: z(oh, ow, 4)), ring(lambda: z(oh, ow, 4))
    for k in range(args.ring):  # real intermediaries for the RCAS-only configurations
        fsr.easu(M(m_in[k]), M(m_mid[k]), con=con)
        fsr.easu(i_in[k], i_mid[k], con=con)
    one = 255 if u8 else 1

    def detour(k):
        """What a caller of the RGBA ABI does for a luma plane today: replicate into RGBA, the RGBA chain, take one channel."""
        x = m_in[k][..., None].expand(ih, iw, 4).contiguous()
        x[..., 3] = one
        fsr.easu(x, i_mid[k], con=con)
        fsr.rcas(i_mid[k], i_out[k], con=rcon)
        return i_out[k][..., 0].contiguous()

    def chain_mono(k):
        fsr.easu(M(m_in[k]), M(m_mid[k]), con=con)
        fsr.rcas(M(m_mid[k]), M(m_out[k]), con=rcon)

    def chain_rgba(k):
        fsr.easu(i_in[k], i_mid[k], con=con)
        fsr.rcas(i_mid[k], i_out[k], con=rcon)

    configs = {
        "rcas_mono": lambda k: fsr.rcas(M(m_mid[k]), M(m_out[k]), con=rcon),
        "rcas_%s" % inter: lambda k: fsr.rcas(i_mid[k], i_out[k], con=rcon),
        "easu_mono": lambda k: fsr.easu(M(m_in[k]), M(m_mid[k]), con=con),
        "easu_%s" % inter: lambda k: fsr.easu(i_in[k], i_mid[k], con=con),
        "chain_mono": chain_mono,
        "chain_%s" % inter: chain_rgba,
        "chain_%s_replicate_slice" % inter: detour,
    }
    # the single-channel chain and the detour compute the same image
    chain_mono(0)
    same = bool(torch.equal(m_out[0], detour(0)))

    def measure(cfgs):
        for fn in cfgs.values():  # warm every kernel on every buffer set
            for k in range(args.ring):
                fn(k)
        torch.cuda.synchronize()
        times = {name: [] for name in cfgs}
        for _ in range(args.windows):
            for name, fn in cfgs.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for c in range(args.calls):
                    fn(c % args.ring)
                e1.record()
                e1.synchronize()
                times[name].append(e0.elapsed_time(e1) * 1000.0 / args.calls)
        return {k: {"median": round(statistics.median(v), 2), "min": round(min(v), 2), "max": round(max(v), 2)} for k, v in times.items()}

    us = measure({k: v for k, v in configs.items() if k.startswith(args.only)})
    doc = {
        "what": "single-channel %s against %s, %dx%d -> %dx%d, default arithmetic, one frame per call; %d calls per window between two events "
                "on one stream, %d windows per configuration, the configurations alternating, each on a ring of %d buffer sets"
                % ((("uint8", "RGBA8_UNORM") if u8 else ("fp16", "RGBA16F")) + (iw, ih, ow, oh, args.calls, args.windows, args.ring)),
        "device": torch.cuda.get_device_name(0),
        "clocks_and_power_after_the_run": smi(),
        "mono_chain_equals_replicate_slice_chain": same,
        "library": os.path.basename(fsr._lib.LIB_PATH),
        "us_per_call": us,
        "build_id": fsr._lib.build_id(),
    }
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(us, indent=1))
    print("mono == replicate / slice:", same)


if __name__ == "__main__":
    main()
