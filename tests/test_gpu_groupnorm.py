"""GroupNorm(+ReLU) kernels (csrc/norm_elem.hip) against the float64 restatement in tests/groupnorm_restated.py, per element.

Bounds (see groupnorm_restated.check_fwd / check_bwd): y and dx ``|err| <= 2^-8 |ref| + EPS * S`` per element, mean ``EPS_M * max_g|x|``,
rstd ``EPS_R`` relative, dgamma / dbeta / dxsum ``EPS_S * sum|summands|``.  Each bound is 4 x the largest figure measured on an MI355X
over all cases (the margin is for the order of the float atomics, which a few runs do not span).

Measured (the larger of plain and ReLU; atomic: the largest of three runs; excess over the relative term in units of S):

    case            mode       eps(y)  eps(dx)    eps_m    eps_r    eps_s  share left out (ReLU)
    cond0           atomic   5.3e-09  1.3e-07  2.0e-08  3.1e-07  3.9e-07  1.3e-05
    cond0           det      5.3e-09  9.3e-08  2.0e-08  3.1e-07  2.8e-07  1.3e-05
    cond1           atomic   1.2e-08  1.1e-07  3.0e-08  3.4e-07  3.0e-07  1.3e-05
    cond1           det      1.2e-08  1.1e-07  2.6e-08  3.4e-07  3.7e-07  1.3e-05
    cond4           atomic   3.2e-08  5.6e-08  3.2e-08  1.4e-07  3.1e-07  5.2e-05
    cond4           det      4.1e-08  5.6e-08  3.2e-08  1.4e-07  2.9e-07  5.2e-05
    cond16          atomic   2.8e-07  3.0e-07  5.0e-08  8.2e-08  7.8e-07  0.0e+00
    cond16          det      2.8e-07  3.0e-07  5.0e-08  8.2e-08  8.3e-07  0.0e+00
    hw5             atomic   0.0e+00  0.0e+00  2.9e-08  9.0e-08  1.7e-07  0.0e+00
    hw5             det      0.0e+00  0.0e+00  2.9e-08  9.0e-08  1.8e-07  0.0e+00
    hw333_c512      atomic   1.7e-08  3.4e-07  2.9e-08  9.3e-07  9.8e-07  5.9e-06
    hw333_c512      det      1.4e-09  3.4e-07  1.9e-08  9.5e-07  1.2e-06  5.9e-06
    hw40_c2048      atomic   4.7e-08  7.0e-07  2.2e-08  1.8e-06  1.7e-06  6.1e-06
    hw40_c2048      det      4.7e-08  7.0e-07  2.2e-08  1.8e-06  1.7e-06  6.1e-06
    hw9000          atomic   4.1e-08  1.6e-07  7.4e-08  4.8e-07  8.1e-07  2.5e-05
    hw9000          det      4.1e-08  1.5e-07  4.3e-08  2.2e-07  3.0e-07  2.5e-05
    ml4             atomic   2.2e-08  7.1e-08  2.7e-08  5.4e-07  4.8e-07  1.5e-05
    ml4             det      2.9e-08  7.1e-08  2.7e-08  4.8e-07  2.1e-07  1.5e-05
    ml_small_first  atomic   6.8e-09  9.1e-08  2.9e-08  5.9e-07  3.5e-07  0.0e+00
    ml_small_first  det      0.0e+00  3.4e-08  3.4e-08  5.9e-07  2.4e-07  0.0e+00
    ml6             atomic   8.9e-09  7.9e-10  1.7e-08  1.9e-07  1.9e-07  0.0e+00
    ml6             det      8.9e-09  3.1e-09  1.7e-08  1.9e-07  1.9e-07  0.0e+00
    ml_cpg16        atomic   2.4e-08  4.8e-07  3.8e-08  1.0e-06  5.5e-07  1.8e-05
    ml_cpg16        det      2.4e-08  3.9e-07  3.8e-08  1.1e-06  5.9e-07  1.8e-05
    ml_zero_group   atomic   1.4e-09  7.7e-08  3.4e-08  5.2e-07  2.9e-07  7.1e-06
    ml_zero_group   det      1.4e-09  5.7e-08  2.3e-08  4.2e-07  3.4e-07  7.1e-06

Largest: eps 7.0e-7, eps_m 7.4e-8, eps_r 1.8e-6, eps_s 1.7e-6; the bounds below are 4 x those, all under the ceilings of
groupnorm_restated (1e-4 / 1e-4 / 1e-5 up to mean/std 4).  The single-level cases were measured in deterministic mode as well.

These are the figures of statistics summed about a per-group pivot (gn_pivot in norm_elem.hip).  With plain sums of x and x^2, as the
kernels formed them before, the same measurement gave eps_r 2.6e-5 and eps_s 1.9e-5 (dgamma inherits rstd's error through xhat) for
cond16, eps(dx) 1.0e-5, eps(y) 1.6e-6 - the eps_s ceiling of 1e-5 was not met - and eps_r 2.1e-6 / eps_s 1.5e-6 for cond4.

With ReLU, an element whose mask may fall on either side (|z| <= 1e-5) moves dbeta of its channel and, through m1, every dx of its group
(one such element of cond1, masked differently from the reference in two of three atomic runs, measured dbeta 8.4e-3 and dx 2.7e-4
in these units): check_bwd takes what those elements can move off the error first; see there.
"""
import ctypes
import os
import subprocess
import sys

import pytest
import torch

import groupnorm_restated as GR

pytestmark = pytest.mark.gpu

# 4 x the largest measured figure of the docstring's table, for every case
EPS = 4 * 7.0e-7
EPS_M = 4 * 7.4e-8
EPS_R = 4 * 1.8e-6
EPS_S = 4 * 1.7e-6


def _bounds(name):
    r = GR.CASES[name][4]
    assert EPS <= GR.EPS_CEIL[r] and EPS_R <= GR.EPS_R_CEIL[r] and EPS_S <= GR.EPS_S_CEIL
    return EPS, EPS_M, EPS_R, EPS_S


def _start(C, cuda):
    g = torch.Generator().manual_seed(7)
    return [torch.randn(C, generator=g).to(cuda) for _ in range(3)]


def run_case(name, relu, cuda, det=False, single=False):
    """One forward and one backward of the case through the bf16 entry points (``single``: the one-level wrappers); dgamma / dbeta /
    dxsum start from random values.  Returns everything the kernels wrote, on the CPU, and the start values."""
    from slenderobjdet_amd.layers import functional as HF

    (xs, dys, gamma, beta, G), ref = GR.case(name, relu)
    xd, dyd = [x.to(cuda).bfloat16() for x in xs], [d.to(cuda).bfloat16() for d in dys]
    gm, bt = gamma.to(cuda), beta.to(cuda)
    start = _start(ref.C, cuda)
    dg, db, dsum = [s.clone() for s in start]
    was = HF.DETERMINISTIC
    HF.DETERMINISTIC = det
    try:
        if single:
            y, stats = HF.groupnorm_fwd(xd[0], gm, bt, G, 1e-5, relu)
            dx = HF.groupnorm_bwd(dyd[0], xd[0], gm, bt, stats, G, dg, db, relu, dxsum=dsum)
            ys, dxs, stats = [y], [dx], stats.unsqueeze(0)
        else:
            ys, stats = HF.groupnorm_fwd_ml(xd, gm, bt, G, 1e-5, relu)
            dxs = HF.groupnorm_bwd_ml(dyd, xd, gm, bt, stats, G, dg, db, relu, dxsum=dsum)
        torch.cuda.synchronize()
    finally:
        HF.DETERMINISTIC = was
    out = ([y.float().cpu() for y in ys], stats.cpu(), [d.float().cpu() for d in dxs], dg.cpu(), db.cpu(), dsum.cpu())
    return out, [s.cpu() for s in start]


def check(name, relu, out, start, what):
    """Prints the run's figures (pytest -s shows them: that is how the docstring's table was taken), then asserts the bounds."""
    ref = GR.case(name, relu)[1]
    assert ref.exclusions_ok()
    eps, eps_m, eps_r, eps_s = _bounds(name)
    ys, stats, dxs, dg, db, dsum = out
    f = GR.check_fwd(ref, ys, stats)
    b = GR.check_bwd(ref, dxs, dg, db, dsum, start=start)
    print(what, name, "relu" if relu else "plain", {k: "%.2e" % v for k, v in {**f, **b}.items()})
    GR.check_fwd(ref, ys, stats, eps=eps, eps_m=eps_m, eps_r=eps_r, what=what)
    GR.check_bwd(ref, dxs, dg, db, dsum, start=start, eps=eps, eps_s=eps_s, what=what)


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("name", list(GR.SINGLE))
def test_single_level(cuda, name, relu):
    out, start = run_case(name, relu, cuda, single=True)
    check(name, relu, out, start, "single level")


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("name", list(GR.MULTI))
def test_multi_level_atomic(cuda, name, relu):
    out, start = run_case(name, relu, cuda)
    check(name, relu, out, start, "multi level, atomic")
    if name == "ml_zero_group":
        _check_zero_group(relu, out)


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("name", list(GR.MULTI))
def test_multi_level_deterministic(cuda, name, relu):
    out, start = run_case(name, relu, cuda, det=True)
    check(name, relu, out, start, "multi level, deterministic")
    again, _ = run_case(name, relu, cuda, det=True)
    for a, b in zip(out, again):      # ys, stats, dxs, dgamma, dbeta, dxsum: bit-identical from run to run
        for s, t in zip(a, b) if isinstance(a, list) else [(a, b)]:
            assert torch.equal(s, t)
    if name == "ml_zero_group":
        _check_zero_group(relu, out)


def _check_zero_group(relu, out):
    """x = 0 over a whole group: y is bf16(relu(beta)) exactly there (dx finite and within the bound: check_bwd)."""
    (xs, _, _, beta, G), ref = GR.case("ml_zero_group", relu)
    l, n, g = GR.ZERO_GROUP
    cpg = ref.C // G
    assert bool((xs[l][n, :, g * cpg:(g + 1) * cpg] == 0).all())
    want = GR.rb(torch.relu(beta) if relu else beta)[g * cpg:(g + 1) * cpg]
    assert torch.equal(out[0][l][n, :, g * cpg:(g + 1) * cpg], want.expand(xs[l].shape[1], cpg))


@pytest.mark.parametrize("relu", [False, True])
def test_apply_from_gathered_sums(cuda, relu):
    """sod_groupnorm_apply_ml as conv_gn_fwd_ml calls it: the statistics buffer comes in holding (sum x, sum x^2) and leaves holding
    (mean, rstd)."""
    from slenderobjdet_amd.layers import functional as HF

    name = GR.FIRST_ML
    (xs, _, gamma, beta, G), ref = GR.case(name, relu)
    N, C = ref.N, ref.C
    x4 = [x.double().reshape(N, x.shape[1], G, C // G) for x in xs]
    sums = torch.stack([torch.stack([x.sum(dim=(1, 3)), (x * x).sum(dim=(1, 3))], dim=-1) for x in x4]).float().to(cuda).contiguous()
    xd = [x.to(cuda).bfloat16() for x in xs]
    ys = [torch.empty_like(x) for x in xd]
    gm, bt = gamma.to(cuda), beta.to(cuda)
    HF.call("sod_groupnorm_apply_ml", len(xd), HF._ptr_arr(xd), HF.ptr(gm), HF.ptr(bt), HF._ptr_arr(ys), HF.ptr(sums),
            N, ctypes.cast(HF._int_arr(ref.hws), ctypes.c_void_p), C, G, 1e-5, 1 if relu else 0, HF.stream_ptr())
    torch.cuda.synchronize()
    eps, eps_m, eps_r, _ = _bounds(name)
    f = GR.check_fwd(ref, [y.float().cpu() for y in ys], sums.cpu())
    print("apply from sums", {k: "%.2e" % v for k, v in f.items()})
    GR.check_fwd(ref, [y.float().cpu() for y in ys], sums.cpu(), eps=eps, eps_m=eps_m, eps_r=eps_r, what="apply from sums")


@pytest.mark.parametrize("mask", [0, 7])
def test_block_order(cuda, mask):
    """SOD_GN_REVERSE is read once per process (the default, 6, is what every test above runs): one child process per mask, one at a time."""
    env = dict(os.environ, SOD_GN_REVERSE=str(mask))
    out = subprocess.run([sys.executable, os.path.abspath(__file__)], capture_output=True, text=True, timeout=180, env=env)
    assert out.returncode == 0, out.stdout[-1500:] + out.stderr[-3000:]
    assert "block order %d ok" % mask in out.stdout


@pytest.mark.parametrize("N,hws,C,G", [(1, [64], 192, 24),        # 24 vectors per pixel do not divide 256
                                       (1, [64], 64, 32),         # 2 channels per group
                                       (1, [64], 4096, 32),
                                       (1, [8] * 7, 256, 32)])    # seven levels
def test_unsupported_shapes_are_rejected(cuda, N, hws, C, G):
    from slenderobjdet_amd._C import SlenderHipError
    from slenderobjdet_amd.layers import functional as HF

    xs = [torch.zeros(N, hw, C, device=cuda, dtype=torch.bfloat16) for hw in hws]
    gamma, beta = torch.ones(C, device=cuda), torch.zeros(C, device=cuda)
    stats = torch.zeros(len(hws), N, G, 2, device=cuda)
    dg, db = torch.zeros(C, device=cuda), torch.zeros(C, device=cuda)
    with pytest.raises(SlenderHipError):
        HF.groupnorm_fwd_ml(xs, gamma, beta, G, 1e-5, True)
    with pytest.raises(SlenderHipError):
        HF.groupnorm_bwd_ml(xs, xs, gamma, beta, stats, G, dg, db, True)
    if len(hws) == 1:
        with pytest.raises(SlenderHipError):
            HF.groupnorm_fwd(xs[0], gamma, beta, G, 1e-5, True)
        with pytest.raises(SlenderHipError):
            HF.groupnorm_bwd(xs[0], xs[0], gamma, beta, stats[0], G, dg, db, True)
    torch.cuda.synchronize()
    assert float(dg.abs().sum() + db.abs().sum()) == 0.0      # nothing was launched


if __name__ == "__main__":      # the child of test_block_order
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    dev = torch.device("cuda:0")
    for relu_ in (False, True):
        out_, start_ = run_case(GR.FIRST_ML, relu_, dev)
        check(GR.FIRST_ML, relu_, out_, start_, "block order " + os.environ.get("SOD_GN_REVERSE", "default"))
    print("block order %s ok" % os.environ.get("SOD_GN_REVERSE", "default"))
