#!/usr/bin/env python3
"""The luma-domain NV12 transcode 1920x1080 -> 3840x2160, default arithmetic, one frame per call (tools/nv12_out_bench.py's protocol):

  transcode_luma            fsr1_transcode_luma: EASU on Y, then ONE launch of the RCAS strips and the chroma strips
  transcode_ycbcr_u8        fsr1_transcode_ycbcr through uint8 planes: the RGB-domain transcode it is compared with
  mono_chain_u8             the single-channel uint8 chain alone (EASU + RCAS on the Y plane): what the luma road cannot go below
  easu_mono_u8, rcas_mono_u8  its two dispatches by themselves
  transcode_luma_separate   (with --separate-lib) fsr1_transcode_luma of a library built with tools/experiments_luma/separate_launches.patch: rcas_mono and
                            a chroma-only launch instead of the combined grid — what riding in one grid is worth

  tools/build_variant.sh lumasep "" tools/experiments_luma/separate_launches.patch
  python tools/luma_bench.py --separate-lib variants/libfsr1_lumasep.so --out profiles/luma_1080p_to_4k.json

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
    ap.add_argument("--separate-lib", default=None)
    ap.add_argument("--calls", type=int, default=300)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--ring", type=int, default=8)
    args = ap.parse_args()
    import torch
    from planar_bench import smi
    fsr = importlib.import_module("fidelityfx-fsr_amd")
    product = fsr.load()
    if not torch.cuda.is_available():
        raise SystemExit("luma_bench needs a GPU")
    separate = fsr._lib._open(os.path.abspath(args.separate_lib), fsr._lib.SYMBOLS) if args.separate_lib else None
    iw, ih, ow, oh = 1920, 1080, 3840, 2160
    P, N, M, yc, conv = fsr.Planar, fsr.Nv12, fsr.Mono, fsr.YCbCr.bt709(), fsr.RgbToYCbCr.bt709()
    m, bias = torch.from_numpy(yc.m).cuda(), torch.from_numpy(yc.bias).cuda()

    # frame 0 of the synthetic sequence as an NV12 surface (tools/nv12_bench.py)
    rgb = torch.from_numpy(fsr.frames.synthetic_frame(iw, ih, k=0)).cuda()[..., :3].float()
    ycc = ((rgb - bias) @ torch.linalg.inv(m).T).round_().clamp_(0, 255)
    chroma = ycc[..., 1:].view(ih // 2, 2, iw // 2, 2, 2).mean(dim=(1, 3)).round_()
    nv12 = torch.cat([ycc[..., 0], chroma.reshape(ih // 2, iw)], 0).to(torch.uint8)

    def ring(make):
        return [make() for _ in range(args.ring)]

    surf = lambda: torch.zeros(oh * 3 // 2, ow, dtype=torch.uint8, device="cuda")  # noqa: E731
    n_in, on = ring(nv12.clone), ring(surf)
    m1, m3 = ring(lambda: torch.zeros(oh, ow, dtype=torch.uint8, device="cuda")), ring(lambda: torch.zeros(3, oh, ow, dtype=torch.uint8, device="cuda"))

    def luma(lib):
        def call(k):
            fsr._lib._lib = lib  # (what _lib.test_hooks does for the test library)
            try:
                return fsr.transcode_luma(N(n_in[k]), M(m1[k]), N(on[k]), sharpness=0.25)
            finally:
                fsr._lib._lib = product
        return call

    def chain(k):
        fsr.easu(M(n_in[k][:ih]), M(m1[k]))
        return fsr.rcas(M(m1[k]), M(on[k][:oh]), sharpness=0.25)

    configs = {
        "transcode_luma": luma(product),
        "transcode_ycbcr_u8": lambda k: fsr.transcode_ycbcr(N(n_in[k]), P(m3[k]), N(on[k]), yc, conv, sharpness=0.25),
        "mono_chain_u8": chain,
        "easu_mono_u8": lambda k: fsr.easu(M(n_in[k][:ih]), M(m1[k])),
        "rcas_mono_u8": lambda k: fsr.rcas(M(m1[k]), M(on[k][:oh]), sharpness=0.25),
    }
    if separate is not None:
        configs["transcode_luma_separate"] = luma(separate)
    for fn in configs.values():  # warm every kernel on every buffer set
        for k in range(args.ring):
            fn(k)
    torch.cuda.synchronize()
    same = None
    if separate is not None:  # the two forms store the same surface
        a = configs["transcode_luma"](0).t.clone()
        same = bool(torch.equal(a, configs["transcode_luma_separate"](0).t))
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
        "what": "NV12 -> NV12 %dx%d -> %dx%d in the luma domain (fsr1_transcode_luma) against the RGB-domain transcode through uint8 planes and the "
                "single-channel uint8 chain, default arithmetic, siting LEFT, one frame per call; %d calls per window between two events on one "
                "stream, %d windows per configuration, the configurations alternating, a ring of %d buffer sets"
                % (iw, ih, ow, oh, args.calls, args.windows, args.ring),
        "device": torch.cuda.get_device_name(0),
        "clocks_and_power_after_the_run": smi(),
        "combined_and_separate_launches_store_the_same_surface": same,
        "us_per_call": {k: {"median": round(statistics.median(v), 2), "min": round(min(v), 2), "max": round(max(v), 2)} for k, v in times.items()},
        "build_id": fsr._lib.build_id(),
    }
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc["us_per_call"], indent=1))


if __name__ == "__main__":
    main()
