"""Remainder ("tail") launches of the split conv dispatches of the FCOS R50 step: what they cost, per shape.

A dispatch that the 256x256 kernel takes with a little more than a whole number of rounds of tiles is split: whole rounds on the 256x256
kernel, the remainder in a second launch of the 128x128-family kernel (csrc/conv_dispatch.hip).  This tool

  1. runs one serial training step of the benchmark model (batch 16, 800 x 1344) with the library's per-dispatch recording on and takes
     from it every split forward / data-gradient dispatch (shape, count per step) - the shapes come from the model, not from a list;
     also the un-split 128x128 dispatches whose grid is 1.0 - 1.25 rounds of two workgroups per CU (information only);
  2. re-runs each of those shapes stand-alone (random operands, bias + ReLU forward / plain data gradient; the towers without their
     GroupNorm statistics), `--reps` times, with one hipEvent pair around the main launch and one around the remainder launch
     (sod_conv_prof_enable(2)), and prints min / median / max of both and the sum of the remainder time per step;
  3. with --calibrate: remainders of chosen sizes (sod_conv_set_tail_split) on every remainder tile, to fill the cost table of
     conv_dispatch.hip (us per 64-deep K-step with k workgroups per CU).

    python tools/bench_conv_tails.py --tail 0 --calibrate      # the 128x128 remainder of every split (the behaviour before the tile choice)
    python tools/bench_conv_tails.py --tail 1                  # the chosen tiles
"""
import argparse
import ctypes
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from slenderobjdet_amd import _C  # noqa: E402
from slenderobjdet_amd.layers import functional as HF  # noqa: E402

TILE_CODES = {12812864: (128, 128, 2), 6412864: (64, 128, 3), 6406464: (64, 64, 4), 36406464: (64, 64, 3)}      # code: BQ, BP, workgroups per CU
dev = torch.device("cuda:0")


def collect(n):
    """(main ms, variant, frac, mode, tail ms, tail variant) of the n dispatches recorded since the last call."""
    f, i = (ctypes.c_float * max(n, 1)), (ctypes.c_int * max(n, 1))
    ms, var, frac, mode, tms, tvar = f(), i(), f(), i(), f(), i()
    lib = _C.load()
    got_t = lib.sod_conv_prof_collect_tails(tms, tvar, n)
    got = lib.sod_conv_prof_collect(ms, var, frac, mode, n)
    assert got == n and got_t == n, (got, got_t, n)
    return [(ms[j], var[j], frac[j], mode[j], tms[j], tvar[j]) for j in range(n)]


def step_dispatches(batch, height, width):
    """One serial step of the benchmark model -> [(kind, desc, variant, frac)] of its forward / data-gradient conv dispatches."""
    from bench import make_cfg, train_step
    from slenderobjdet_amd.data import SyntheticCocoBatches
    from slenderobjdet_amd.modeling import build_model
    from slenderobjdet_amd.modeling.meta_arch import fcos as fcos_mod
    from slenderobjdet_amd.solver import build_optimizer

    cfg = make_cfg(50, "fcos")
    torch.manual_seed(1)
    model = build_model(cfg)
    model.train()
    opt = build_optimizer(cfg, model)
    loader = SyntheticCocoBatches(batch, height, width, rank=0, device=dev, pool=2)
    HF.WGRAD_SIDE_STREAM = False
    fcos_mod.TOWER_STREAMS = False
    for _ in range(2):
        train_step(model, opt, next(loader))
    torch.cuda.synchronize()
    rec = []
    HF.PROFILE, HF.PROFILE_KINDS, HF.PROFILE_LIB = rec, None, True
    _C.call("sod_conv_prof_enable", 1)
    train_step(model, opt, next(loader))
    torch.cuda.synchronize()
    _C.call("sod_conv_prof_enable", 0)
    HF.PROFILE, HF.PROFILE_LIB = None, False
    lib_rows = [r for r in rec if r[2] is None]
    rows = collect(len(lib_rows))
    out = []
    for (kind, _fl, _e0, _e1, desc, _v), (_ms, var, frac, mode, _tms, _tvar) in zip(lib_rows, rows):
        assert {"conv_fwd": 0, "conv_dgrad": 1, "conv_wgrad": 2}[kind] == mode
        if kind != "conv_wgrad":
            out.append((kind, desc, var, frac))
    del model, opt, loader
    torch.cuda.empty_cache()
    return out


def geometry(kind, desc):
    """desc of layers/functional.py -> (N, [(H, W)] input side of the convolution, C, K, R, stride, output pixels, Nout, Kred)."""
    if desc[0] == "ml":
        _, N, hs, C, K, R, stride, ws = desc
        hw = list(zip(hs, ws))
    else:
        N, H, W, C, K, R, stride = desc[:7]
        hw = [(H, W)]
    pad = R // 2
    outs = [HF.conv_out_size(h, w, R, R, stride, pad, 1) for h, w in hw]
    if kind == "conv_fwd":
        pix, nout, kred = [N * ho * wo for ho, wo in outs], K, R * R * C
    else:      # the data gradient's GEMM rows are the INPUT pixels, its contraction runs over the K channels of dY
        pix, nout, kred = [N * h * w for h, w in hw], C, R * R * K
    return N, hw, C, K, R, stride, pix, nout, kred


def make_call(kind, desc):
    N, hw, C, K, R, stride, _pix, _nout, _kred = geometry(kind, desc)
    pad = R // 2
    g = torch.Generator(device=dev).manual_seed(3)
    if kind == "conv_fwd":
        xs = [torch.randn(N, h, w, C, device=dev, generator=g).bfloat16() for h, w in hw]
        wgt = (torch.randn(K, R, R, C, device=dev, generator=g) * 0.05).bfloat16()
        bias = torch.randn(K, device=dev, generator=g)
        if desc[0] == "ml":
            return lambda: HF.conv2d_fwd_ml(xs, wgt, bias, stride, pad, 1, relu=False)
        return lambda: HF.conv2d_fwd(xs[0], wgt, bias, stride=stride, pad=pad, relu=True)
    dys = [torch.randn(N, *HF.conv_out_size(h, w, R, R, stride, pad, 1), K, device=dev, generator=g).bfloat16() for h, w in hw]
    wt = (torch.randn(C, R, R, K, device=dev, generator=g) * 0.05).bfloat16()
    if desc[0] == "ml":
        return lambda: HF.conv2d_dgrad_ml(dys, wt, hw, stride, pad, 1)
    return lambda: HF.conv2d_dgrad(dys[0], wt, hw[0], stride, pad, 1)


def run_timed(fn, reps):
    """reps stand-alone dispatches -> ([main us], [tail us], tail code, variant)."""
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    _C.call("sod_conv_prof_enable", 2)
    for _ in range(reps):
        fn()
        torch.cuda.synchronize()
    _C.call("sod_conv_prof_enable", 0)
    rows = collect(reps)
    return [r[0] * 1e3 for r in rows], [r[4] * 1e3 for r in rows], rows[0][5], rows[0][1]


def run_plain(fn, reps):
    for _ in range(2):
        fn()
    out = []
    for _ in range(reps):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        s.record(); fn(); e.record()
        torch.cuda.synchronize()
        out.append(s.elapsed_time(e) * 1e3)
    return out


def mmm(v):
    return f"{min(v):7.1f} {statistics.median(v):7.1f} {max(v):7.1f}"


def shape_str(kind, desc):
    N, hw, C, K, R, stride, _pix, _nout, _kred = geometry(kind, desc)
    lv = "+".join(f"{h}x{w}" for h, w in hw)
    return f"{'fwd  ' if kind == 'conv_fwd' else 'dgrad'} N={N} {lv} {C}->{K} {R}x{R}/{stride}"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tail", type=int, default=1, help="sod_conv_set_tail_tile: 0 = the ordinary rules' 128x128 remainder, 1 = the chosen tile, or a tile code")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--height", type=int, default=800)
    ap.add_argument("--width", type=int, default=1333)
    ap.add_argument("--calibrate", action="store_true")
    ap.add_argument("--out", default=None, help="also write the tables to this file")
    args = ap.parse_args()
    assert args.reps >= 5
    lines = []

    def emit(s=""):
        print(s, flush=True)
        lines.append(s)

    torch.cuda.set_device(0)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    _C.call("sod_conv_set_tail_tile", args.tail)
    disp = step_dispatches(args.batch, args.height, args.width)
    split, near = {}, {}
    for kind, desc, var, frac in disp:
        _N, _hw, _C2, _K, _R, _s, pix, nout, _kred = geometry(kind, desc)
        if var == 256 and frac < 1.0:
            split[(kind, desc)] = split.get((kind, desc), 0) + 1
        elif var // 100 == 128128:      # 128x128 tile (BK 64 or 32), not split
            blocks = sum((p + 127) // 128 for p in pix) * ((nout + 127) // 128)
            if 1.0 <= blocks / (2.0 * cus) <= 1.25:
                near[(kind, desc, var)] = near.get((kind, desc, var), 0) + 1
    emit(f"# tools/bench_conv_tails.py --tail {args.tail} --reps {args.reps}: {torch.cuda.get_device_name(0)}, {cus} CUs, batch {args.batch}, "
         f"{args.height}x{args.width}; stand-alone runs, us, min / median / max of {args.reps}")
    emit(f"# split dispatches of one FCOS R50 step: {sum(split.values())} ({sum(c for (k, _), c in split.items() if k == 'conv_fwd')} forward, "
         f"{sum(c for (k, _), c in split.items() if k == 'conv_dgrad')} data gradient), {len(split)} distinct shapes")
    emit(f"{'shape':<58} {'n/step':>6} {'Nout':>5} {'Kred':>5} {'tiles':>6} {'rounds':>6} {'rem':>4} {'tail tile':>9}   {'main us (min med max)':>23}   {'tail us (min med max)':>23}")
    tot = {"single": [0.0, 0.0, 0.0], "ml": [0.0, 0.0, 0.0]}
    for (kind, desc), cnt in sorted(split.items(), key=lambda kv: (kv[0][1][0] == "ml", kv[0][0], str(kv[0][1]))):
        _N, _hw, _C2, _K, _R, _s, pix, nout, kred = geometry(kind, desc)
        tiles = sum((p + 255) // 256 for p in pix) * ((nout + 255) // 256)
        main_us, tail_us, tcode, var = run_timed(make_call(kind, desc), args.reps)
        assert var == 256 and tcode != 0, (desc, var, tcode)
        grp = tot["ml" if desc[0] == "ml" else "single"]
        for j, f in enumerate((min, statistics.median, max)):
            grp[j] += cnt * f(tail_us)
        emit(f"{shape_str(kind, desc):<58} {cnt:>6} {nout:>5} {kred:>5} {tiles:>6} {tiles / cus:>6.3f} {tiles % cus:>4} {tcode:>9}   {mmm(main_us)}   {mmm(tail_us)}")
    emit(f"# sum of tail time per step, single-level dispatches (backbone / FPN): min {tot['single'][0]:.1f}  median {tot['single'][1]:.1f}  max {tot['single'][2]:.1f} us")
    emit(f"# sum of tail time per step, multi-level dispatches (towers):          min {tot['ml'][0]:.1f}  median {tot['ml'][1]:.1f}  max {tot['ml'][2]:.1f} us")
    emit()
    emit("# un-split 128x128 dispatches with 1.0 - 1.25 rounds of two workgroups per CU (information only; whole dispatch, torch events)")
    for (kind, desc, var), cnt in sorted(near.items(), key=lambda kv: str(kv[0])):
        _N, _hw, _C2, _K, _R, _s, pix, nout, kred = geometry(kind, desc)
        blocks = sum((p + 127) // 128 for p in pix) * ((nout + 127) // 128)
        t = run_plain(make_call(kind, desc), args.reps)
        emit(f"{shape_str(kind, desc):<58} {cnt:>6} {nout:>5} {kred:>5} blocks {blocks:>5} rounds {blocks / (2.0 * cus):.3f} variant {var}   {mmm(t)}")

    if args.calibrate:
        emit()
        emit("# calibration: remainders of r 256-pixel tiles behind 263 - r main tiles (sod_conv_set_tail_split), N=16 50x84, Nout 256; tail us median")
        emit("# (min max); us/step = median / (K-steps x rounds), k = workgroups per CU, rounds = ceil(workgroups / (k x CUs))")
        for kind, C, R in (("conv_fwd", 256, 3), ("conv_dgrad", 256, 3), ("conv_fwd", 1024, 1)):
            desc = (16, 50, 84, C, 256, R, 1, 0)
            fn = make_call(kind, desc)
            steps = R * R * C // 64
            for r in (7, 16, 26, 32, 48, 64, 96, 122):
                _C.call("sod_conv_set_tail_split", 263 - r)
                row = f"{shape_str(kind, desc):<40} r={r:>3}"
                for code, (bq, bp, per_cu) in TILE_CODES.items():
                    _C.call("sod_conv_set_tail_tile", code)
                    _m, tail_us, tcode, _v = run_timed(fn, args.reps)
                    assert tcode == code, (tcode, code)
                    blocks = -(-(16 * 50 * 84 - (263 - r) * 256) // bp) * (256 // bq)
                    k = min(per_cu, -(-blocks // cus))
                    rounds = -(-blocks // (k * cus))
                    med = statistics.median(tail_us)
                    row += f" | {code}: wg {blocks:>4} k {k} x{rounds} {med:6.1f} ({min(tail_us):.1f} {max(tail_us):.1f}) {med / (steps * rounds):.3f}/step"
                emit(row)
        _C.call("sod_conv_set_tail_split", -1)
    _C.call("sod_conv_set_tail_tile", -1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
