"""tests/groupnorm_restated.py on its own (CPU): the float64 restatement equals ``torch.nn.functional.group_norm`` (+ relu) and autograd
through it; the reference alone meets the conditions on the elements left out of the dx comparison, for every case the GPU tests
use; the comparison accepts the correctly rounded float64 result with eps = 0 and rejects, with every bound at its ceiling, four
answers a subtly wrong kernel could give: m1 dropped, m2 dropped, the ReLU mask taken without beta, and the statistics of the
neighbouring slot of the statistics buffer (the previous level's; in a one-level case the previous (image, group)'s)."""
import pytest
import torch
import torch.nn.functional as F

import groupnorm_restated as GR

ALL = list(GR.CASES)


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("name", ["cond4", "hw333_c512", "ml6"])
def test_restatement_equals_torch_group_norm_and_autograd(name, relu):
    xs, dys, gamma, beta, G = GR.make_inputs(name)
    for x, dy in zip(xs, dys):
        xn = x.double().permute(0, 2, 1).contiguous().requires_grad_(True)      # (N, C, HW)
        gm, bt = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
        ref = F.group_norm(xn, G, gm, bt, 1e-5)
        ref = torch.relu(ref) if relu else ref
        gx, gg, gb = torch.autograd.grad(ref, (xn, gm, bt), dy.double().permute(0, 2, 1))
        y, mean, rstd, z = GR.forward(x, gamma, beta, G, 1e-5, relu)
        dx, dgamma, dbeta, m1, m2 = GR.backward(x, dy, gamma, beta, G, 1e-5, relu)
        for got, want in ((y, ref.detach().permute(0, 2, 1)), (dx, gx.permute(0, 2, 1)), (dgamma, gg), (dbeta, gb)):
            assert (got - want).abs().max().item() <= 1e-12 * want.abs().max().item()
        x4 = x.double().reshape(x.shape[0], x.shape[1], G, -1)
        assert torch.allclose(mean, x4.mean(dim=(1, 3)), rtol=1e-12, atol=0)
        assert torch.allclose(rstd, (x4.var(dim=(1, 3), unbiased=False) + 1e-5).rsqrt(), rtol=1e-12, atol=0)
        assert torch.equal(y, torch.relu(z) if relu else z)


@pytest.mark.parametrize("name", ALL)
def test_the_reference_alone_meets_the_exclusion_conditions(name):
    _, ref = GR.case(name, True)
    share, small = ref.excluded_share()
    assert share <= GR.SHARE_MAX and small == 0, (share, small)
    assert GR.case(name, False)[1].excluded_share() == (0.0, 0)


def _ceilings(name):
    ratio = GR.CASES[name][4]
    return GR.EPS_CEIL[ratio], GR.EPS_R_CEIL[ratio], GR.EPS_S_CEIL


def _shifted_stats(ref):
    """The statistics buffer (L, N, G) read one slot too early: level l gets level l - 1's; with one level, (n, g) gets its predecessor's."""
    mean, rstd = torch.stack(ref.mean), torch.stack(ref.rstd)
    if len(ref.mean) > 1:
        return list(mean.roll(1, 0)), list(rstd.roll(1, 0))
    return [mean.flatten().roll(1).reshape(mean.shape)[0]], [rstd.flatten().roll(1).reshape(rstd.shape)[0]]


def _kernel_like(name, relu, wrong):
    """What a kernel with the named defect would store: float64 arithmetic, outputs rounded to bf16 (sums and statistics to fp32)."""
    (xs, dys, gamma, beta, G), ref = GR.case(name, relu)
    means, rstds = _shifted_stats(ref) if wrong == "stats_shifted" else (ref.mean, ref.rstd)
    g4, b4 = gamma.double().reshape(1, 1, G, -1), beta.double().reshape(1, 1, G, -1)
    ys, dxs = [], []
    dgamma, dbeta = torch.zeros(ref.C, dtype=torch.float64), torch.zeros(ref.C, dtype=torch.float64)
    for x, dy, mean, rstd in zip(xs, dys, means, rstds):
        N, HW, C = x.shape
        rs = rstd.reshape(N, 1, G, 1)
        xh = (x.double().reshape(N, HW, G, -1) - mean.reshape(N, 1, G, 1)) * rs
        z = xh * g4 + b4
        ys.append(GR.rb((torch.relu(z) if relu else z).reshape(N, HW, C)))
        d = dy.double().reshape(N, HW, G, -1)
        if relu:
            d = d * ((xh * g4 > 0) if wrong == "mask_without_beta" else (z > 0))
            if wrong == "near_cut_flipped":      # not wrong: within Z_CUT of the cut either mask is right
                d = torch.where(z.abs() <= GR.Z_CUT, dy.double().reshape(N, HW, G, -1) * (z <= 0), d)
        dgamma += (d * xh).sum(dim=(0, 1)).reshape(C)
        dbeta += d.sum(dim=(0, 1)).reshape(C)
        m1 = 0.0 if wrong == "m1_dropped" else (g4 * d).mean(dim=(1, 3), keepdim=True)
        m2 = 0.0 if wrong == "m2_dropped" else (g4 * d * xh).mean(dim=(1, 3), keepdim=True)
        dxs.append(GR.rb((rs * (g4 * d - m1 - xh * m2)).reshape(N, HW, C)))
    stats = torch.stack([torch.stack(means), torch.stack(rstds)], dim=-1).float()
    dxsum = sum(dx.double().sum(dim=(0, 1)) for dx in dxs)
    return ys, stats, dxs, dgamma.float(), dbeta.float(), dxsum.float()


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("name", ALL)
def test_the_comparison_accepts_the_rounded_reference_and_rejects_wrong_answers(name, relu):
    _, ref = GR.case(name, relu)
    eps, eps_r, eps_s = _ceilings(name)
    # the right answer: per element with eps = 0, sums and statistics within their rounding to fp32
    ys, stats, dxs, dgamma, dbeta, dxsum = _kernel_like(name, relu, None)
    GR.check_fwd(ref, ys, stats, eps=0.0, eps_m=2.0 ** -24, eps_r=2.0 ** -24)
    GR.check_bwd(ref, dxs, dgamma, dbeta, dxsum, eps=0.0, eps_s=2.0 ** -24)
    # dgamma / dbeta / dxsum accumulate: the comparison takes the start values off
    start = [torch.full((ref.C,), v) for v in (1.5, -0.25, 3.0)]
    GR.check_bwd(ref, dxs, dgamma + start[0], dbeta + start[1], dxsum + start[2], start=start, eps=0.0, eps_s=2.0 ** -22)
    with pytest.raises(AssertionError):
        GR.check_bwd(ref, dxs, dgamma, dbeta, dxsum, start=start, eps=eps, eps_s=eps_s)
    # every element within Z_CUT of the ReLU cut masked the other way: as right as the reference
    ys, stats, dxs, dgamma, dbeta, dxsum = _kernel_like(name, relu, "near_cut_flipped")
    GR.check_bwd(ref, dxs, dgamma, dbeta, dxsum, eps=0.0, eps_s=2.0 ** -24)
    for wrong in ("m1_dropped", "m2_dropped", "stats_shifted") + (("mask_without_beta",) if relu else ()):
        ys, stats, dxs, dgamma, dbeta, dxsum = _kernel_like(name, relu, wrong)
        with pytest.raises(AssertionError):      # the per-element dx bound alone
            GR.check_bwd(ref, dxs, dgamma, dbeta, dxsum, eps=eps)
        if wrong == "stats_shifted":
            with pytest.raises(AssertionError):  # y alone
                GR.check_fwd(ref, ys, stats, eps=eps)
            with pytest.raises(AssertionError):
                GR.check_fwd(ref, ys, stats, eps_m=1e-5)
            with pytest.raises(AssertionError):
                GR.check_fwd(ref, ys, stats, eps_r=eps_r)
        if wrong == "mask_without_beta":
            with pytest.raises(AssertionError):  # and the channel sums alone
                GR.check_bwd(ref, dxs, dgamma, dbeta, None, eps_s=eps_s)
