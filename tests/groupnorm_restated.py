"""A float64 restatement of GroupNorm(+ReLU) forward and backward for the operator-level tests, CPU only, and the per-element
comparison the tests hold the HIP kernels (csrc/norm_elem.hip) to.  No import of the product.

Tensors are (N, HW, C) per level (NHWC with the pixels flattened); a group is ``C // G`` adjacent channels of one image of one level.
The functions work on the values the kernel sees (x and dy already rounded to bf16, gamma / beta fp32), in float64 throughout:

    mean, var (two-pass), rstd = 1 / sqrt(var + eps), xhat = (x - mean) * rstd, z = xhat * gamma + beta, y = relu(z) or z
    d = dy * [z > 0] (or dy), dgamma = sum d * xhat, dbeta = sum d, m1 = mean_g(gamma * d), m2 = mean_g(gamma * d * xhat),
    dx = rstd * (gamma * d - m1 - xhat * m2)

The comparison (:func:`check_fwd`, :func:`check_bwd`) is per element, ``|got - ref| <= 2^-8 |ref| + eps * S`` with ``S`` the scale of
the element's group: the first term is half a bf16 ulp of the stored value at its worst (one rounding of a value that may sit next
to a rounding boundary), the second is what the fp32 arithmetic before the rounding may add, in units of the group's largest
value.  Statistics and channel sums have fixed-form bounds; see the two functions.  Both return what they measured, so a test can
record the figures before it asserts.

tests/test_groupnorm_restated_host.py pins the restatement to ``torch.nn.functional.group_norm`` and its autograd, and shows that the
comparison rejects four kinds of wrong answer for every case below.
"""
import functools

import torch

REL = 2.0 ** -8          # the relative term of the per-element bound
Z_CUT = 1e-5             # |z| up to which the ReLU mask may fall on either side (forward: x * sc + sh, backward: xhat * gamma + beta)
SHARE_MAX = 1e-4         # largest share of elements a case may leave out of the dx comparison for that reason ...
SMALL_GROUP = 1000       # ... and none at all where a group has fewer elements than this
# ceilings of the bounds (tests/test_gpu_groupnorm.py sets the bounds themselves, from measurements, below these)
EPS_CEIL = {0: 1e-4, 1: 1e-4, 4: 1e-4, 16: 2e-3}
EPS_R_CEIL = {0: 1e-4, 1: 1e-4, 4: 1e-4, 16: 2e-3}
EPS_S_CEIL = 1e-5

# name -> (N, [HW per level], C, G, mean/std)
SINGLE = {
    "cond0": (2, [300], 256, 32, 0), "cond1": (2, [300], 256, 32, 1), "cond4": (2, [300], 256, 32, 4), "cond16": (2, [300], 256, 32, 16),
    # the backward passes' landing buffers at their edges: fewer pixels than one trip, one row per wave, one row per block, many blocks
    "hw5": (2, [5], 256, 32, 1), "hw333_c512": (1, [333], 512, 32, 1), "hw40_c2048": (2, [40], 2048, 32, 1), "hw9000": (2, [9000], 256, 32, 1),
}
MULTI = {
    "ml4": (3, [851, 228, 60, 15], 256, 32, 1),                 # no level a multiple of 64 pixels
    "ml_small_first": (2, [15, 851, 60], 256, 32, 1),           # pixels per block come from a small hw[0]
    "ml6": (1, [1, 7, 64, 65, 129, 300], 128, 16, 1),           # six levels, a one-pixel level, 16 rows per trip
    "ml_cpg16": (2, [200, 77], 512, 32, 1),                     # 16 channels per group: two channel vectors per group
    "ml_zero_group": (2, [200, 77], 256, 32, 1),                # x = 0 over the whole group ZERO_GROUP
}
CASES = {**SINGLE, **MULTI}
ZERO_GROUP = (1, 1, 5)      # (level, image, group) of "ml_zero_group"
SEED = {name: 100 + i for i, name in enumerate(CASES)}
FIRST_ML = "ml4"


def rb(t):
    """Round to bf16 and back to fp32: the storage precision of the kernel's activations."""
    return t.to(torch.bfloat16).to(torch.float32)


def _grp(t, G):
    N, HW, C = t.shape
    return t.reshape(N, HW, G, C // G)


def _cg(v, G):
    """(C,) per-channel vector -> (1, 1, G, cpg)"""
    return v.reshape(1, 1, G, -1)


def forward(x, gamma, beta, G, eps=1e-5, relu=False):
    """x (N, HW, C); returns y, mean (N, G), rstd (N, G), z (the pre-activation), all float64."""
    x4 = _grp(x.double(), G)
    mean = x4.mean(dim=(1, 3), keepdim=True)
    var = ((x4 - mean) ** 2).mean(dim=(1, 3), keepdim=True)
    rstd = 1.0 / torch.sqrt(var + eps)
    z = (x4 - mean) * rstd * _cg(gamma.double(), G) + _cg(beta.double(), G)
    y = torch.relu(z) if relu else z
    return y.reshape(x.shape), mean.reshape(x.shape[0], G), rstd.reshape(x.shape[0], G), z.reshape(x.shape)


def backward(x, dy, gamma, beta, G, eps=1e-5, relu=False, mask=None):
    """Returns dx (N, HW, C), dgamma (C,), dbeta (C,), m1 (N, G), m2 (N, G).  ``mask`` replaces the ReLU mask ``z > 0``."""
    N, HW, C = x.shape
    _, mean, rstd, z = forward(x, gamma, beta, G, eps, relu)
    x4, g4 = _grp(x.double(), G), _cg(gamma.double(), G)
    mean4, rstd4 = mean.reshape(N, 1, G, 1), rstd.reshape(N, 1, G, 1)
    xh = (x4 - mean4) * rstd4
    d = _grp(dy.double(), G)
    if relu:
        d = d * _grp((z > 0) if mask is None else mask, G)
    dgamma = (d * xh).sum(dim=(0, 1)).reshape(C)
    dbeta = d.sum(dim=(0, 1)).reshape(C)
    m1 = (g4 * d).mean(dim=(1, 3), keepdim=True)
    m2 = (g4 * d * xh).mean(dim=(1, 3), keepdim=True)
    dx = rstd4 * (g4 * d - m1 - xh * m2)
    return dx.reshape(N, HW, C), dgamma, dbeta, m1.reshape(N, G), m2.reshape(N, G)


# ------------------------------------------------------------------ cases
def make_inputs(name):
    """The case's inputs: xs, dys (lists of (N, HW, C) fp32 holding bf16 values), gamma, beta (fp32), G.

    x = rb(sigma_l * randn + mu_g) with mu_g = +- ratio * sigma_l (the sign alternates from group to group, so neighbouring groups
    and, through sigma_l = 2 * 0.8^l, neighbouring levels have different statistics); dy = rb(0.5 randn + 0.7 + 0.5 tanh(x - mu_g)),
    which has a mean and is correlated with x: m1 and m2 are of the order of gamma, not of 1 / sqrt(elements per group)."""
    N, hws, C, G, ratio = CASES[name]
    g = torch.Generator().manual_seed(SEED[name])
    gamma = torch.rand(C, generator=g) + 0.5
    beta = torch.randn(C, generator=g) * 0.2
    sign = (1.0 - 2.0 * (torch.arange(G) % 2)).repeat_interleave(C // G)
    xs, dys = [], []
    for l, hw in enumerate(hws):
        sigma = 2.0 * 0.8 ** l
        mu = ratio * sigma * sign
        if name == "ml_zero_group" and l == ZERO_GROUP[0]:
            mu = mu.repeat(N, 1)
            lo = ZERO_GROUP[2] * (C // G)
            mu[ZERO_GROUP[1], lo:lo + C // G] = 0.0
            mu = mu.reshape(N, 1, C)
        x = sigma * torch.randn(N, hw, C, generator=g) + mu
        if name == "ml_zero_group" and l == ZERO_GROUP[0]:
            x[ZERO_GROUP[1], :, lo:lo + C // G] = 0.0
        x = rb(x)
        dys.append(rb(0.5 * torch.randn(N, hw, C, generator=g) + 0.7 + 0.5 * torch.tanh(x - mu)))
        xs.append(x)
    return xs, dys, gamma, beta, G


class Reference:
    """Everything the comparison needs of one case, computed once: per level y / mean / rstd / z / dx / m1 / m2 and the scales S, over
    all levels dgamma / dbeta and the sums of the absolute values of their summands."""

    def __init__(self, xs, dys, gamma, beta, G, eps=1e-5, relu=False):
        self.G, self.relu, self.eps = G, relu, eps
        self.N, self.C = xs[0].shape[0], xs[0].shape[2]
        self.hws = [x.shape[1] for x in xs]
        g4, b4 = _cg(gamma.double(), G), _cg(beta.double(), G)
        self.y, self.mean, self.rstd, self.z, self.dx, self.m1, self.m2 = [], [], [], [], [], [], []
        self.s_y, self.s_dx, self.xmax = [], [], []
        self.dgamma = torch.zeros(self.C, dtype=torch.float64)
        self.dbeta = torch.zeros(self.C, dtype=torch.float64)
        self.abs_dgamma, self.abs_dbeta = torch.zeros_like(self.dgamma), torch.zeros_like(self.dbeta)
        # what the elements whose mask may fall on either side (near_cut) can move: dgamma / dbeta of their channel by |dy * xhat| / |dy|,
        # and through m1 and m2 every dx of their group by rstd * (sum|gamma dy| + |xhat| * sum|gamma dy xhat|) / (elements per group)
        self.flip_dgamma, self.flip_dbeta = torch.zeros_like(self.dgamma), torch.zeros_like(self.dbeta)
        self.flip_dx = []
        for x, dy in zip(xs, dys):
            N, HW, C = x.shape
            y, mean, rstd, z = forward(x, gamma, beta, G, eps, relu)
            dx, dg, db, m1, m2 = backward(x, dy, gamma, beta, G, eps, relu)
            xh = (_grp(x.double(), G) - mean.reshape(N, 1, G, 1)) * rstd.reshape(N, 1, G, 1)
            d = _grp(dy.double(), G) * (_grp(z > 0, G) if relu else 1.0)
            self.abs_dgamma += (d * xh).abs().sum(dim=(0, 1)).reshape(C)
            self.abs_dbeta += d.abs().sum(dim=(0, 1)).reshape(C)
            self.dgamma += dg
            self.dbeta += db
            # scale of a group: y: max|gamma| * max|xhat| + max|beta|; dx: rstd * max|gamma * dy|
            self.s_y.append(g4.abs().amax(dim=3).reshape(1, G) * xh.abs().amax(dim=(1, 3)) + b4.abs().amax(dim=3).reshape(1, G))
            self.s_dx.append(rstd * (g4 * _grp(dy.double(), G)).abs().amax(dim=(1, 3)))
            self.xmax.append(_grp(x.double(), G).abs().amax(dim=(1, 3)))
            for lst, v in zip((self.y, self.mean, self.rstd, self.z, self.dx, self.m1, self.m2), (y, mean, rstd, z, dx, m1, m2)):
                lst.append(v)
            cut = _grp(self.near_cut(len(self.z) - 1), G)
            if bool(cut.any()):
                dy4 = _grp(dy.double(), G).abs() * cut
                self.flip_dgamma += (dy4 * xh.abs()).sum(dim=(0, 1)).reshape(C)
                self.flip_dbeta += dy4.sum(dim=(0, 1)).reshape(C)
                f1 = (g4.abs() * dy4).mean(dim=(1, 3), keepdim=True)
                f2 = (g4.abs() * dy4 * xh.abs()).mean(dim=(1, 3), keepdim=True)
                self.flip_dx.append((rstd.reshape(N, 1, G, 1) * (f1 + xh.abs() * f2)).reshape(N, HW, C))
            else:
                self.flip_dx.append(None)

    def near_cut(self, l):
        """Elements of level l whose ReLU mask may legitimately differ between kernel and reference."""
        if not self.relu:
            return torch.zeros_like(self.z[l], dtype=torch.bool)
        return self.z[l].abs() <= Z_CUT

    def excluded_share(self):
        """(share of all elements left out of the dx comparison, the same over the levels with small groups only)"""
        cpg = self.C // self.G
        tot = sum(z.numel() for z in self.z)
        cut = [int(self.near_cut(l).sum()) for l in range(len(self.z))]
        small = sum(c for c, hw in zip(cut, self.hws) if hw * cpg < SMALL_GROUP)
        return sum(cut) / tot, small

    def exclusions_ok(self):
        share, small = self.excluded_share()
        return share <= SHARE_MAX and small == 0


@functools.lru_cache(maxsize=None)
def case(name, relu):
    """(inputs, Reference) of a named case, shared by every test that needs it; treat both as read-only."""
    inp = make_inputs(name)
    return inp, Reference(*inp, relu=relu)


# ------------------------------------------------------------------ the comparison
def _per_group(t, G):
    """(N, G) -> broadcastable against (N, HW, G, cpg)"""
    return t.reshape(t.shape[0], 1, G, 1)


def _excess(got, ref, scale, G, keep=None, slack=None):
    """max over elements of (|got - ref| - REL * |ref| - slack) / S, at least 0; elements where ``keep`` is False are left out."""
    err = (got.double() - ref).abs() - REL * ref.abs()
    if slack is not None:
        err = err - (1 + REL) * slack
    err = _grp(err, G) / _per_group(scale, G)
    if keep is not None:
        err = torch.where(_grp(keep, G), err, torch.zeros_like(err))
    return max(float(err.max()), 0.0) if err.numel() else 0.0


def check_fwd(ref, ys, stats, eps=None, eps_m=None, eps_r=None, what="groupnorm fwd"):
    """ys: per level (N, HW, C) (any float dtype, CPU); stats: (L, N, G, 2) = (mean, rstd).  Returns the measured figures
    {"y": excess in units of S, "mean": |err| / max_g|x|, "rstd": relative error}, each the maximum over all levels, and asserts
    every one whose bound is given: per element |y - ref| <= 2^-8 |ref| + eps * S; |mean err| <= eps_m * max_g|x| (a group that is
    zero throughout must have mean 0); |rstd err| <= eps_r * rstd."""
    out = {"y": 0.0, "mean": 0.0, "rstd": 0.0}
    for l in range(len(ref.y)):
        y = ys[l].reshape(ref.y[l].shape)
        assert bool(torch.isfinite(y.double()).all()), f"{what}: level {l}: y is not finite"
        out["y"] = max(out["y"], _excess(y, ref.y[l], ref.s_y[l], ref.G))
        st = stats[l].double().reshape(ref.N, ref.G, 2)
        merr = (st[..., 0] - ref.mean[l]).abs()
        xm = ref.xmax[l]
        assert bool((merr[xm == 0] == 0).all()), f"{what}: level {l}: mean of an all-zero group is not 0"
        out["mean"] = max(out["mean"], float((merr / xm.clamp_min(1e-300))[xm > 0].max()))
        out["rstd"] = max(out["rstd"], float(((st[..., 1] - ref.rstd[l]).abs() / ref.rstd[l]).max()))
    for key, bound in (("y", eps), ("mean", eps_m), ("rstd", eps_r)):
        if bound is not None:
            assert out[key] <= bound, f"{what}: {key}: {out[key]:.3e} > {bound:.3e}"
    return out


def check_bwd(ref, dxs, dgamma, dbeta, dxsum=None, start=None, eps=None, eps_s=None, what="groupnorm bwd"):
    """dxs: per level (N, HW, C); dgamma / dbeta / dxsum (C,) as the kernel left them; ``start``: what (dgamma, dbeta, dxsum) held
    before the call (the kernel accumulates; default zeros).  Returns {"dx": excess in units of S over the compared elements,
    "dgamma", "dbeta", "dxsum": |err| / sum|summands|, "share": share of elements left out} and asserts those whose bound is given.
    dxsum is held to the float64 sum of the dx the kernel stored (bf16), with sum|dx stored| as its scale.
    Elements with |z| <= Z_CUT (ReLU only) are left out of the dx comparison; dx must be finite everywhere.  Either mask is right for
    such an element, so what its two choices differ by (Reference.flip_*) is taken off the error of its channel's dgamma / dbeta and
    of its group's dx before the bounds apply; where no element is that close to the cut, nothing is taken off."""
    out = {"dx": 0.0}
    sum_dx = torch.zeros(ref.C, dtype=torch.float64)
    abs_dx = torch.zeros(ref.C, dtype=torch.float64)
    for l in range(len(ref.dx)):
        dx = dxs[l].reshape(ref.dx[l].shape).double()
        assert bool(torch.isfinite(dx).all()), f"{what}: level {l}: dx is not finite"
        out["dx"] = max(out["dx"], _excess(dx, ref.dx[l], ref.s_dx[l], ref.G, keep=~ref.near_cut(l), slack=ref.flip_dx[l]))
        sum_dx += dx.sum(dim=(0, 1))
        abs_dx += dx.abs().sum(dim=(0, 1))
    out["share"] = ref.excluded_share()[0]
    s0 = [torch.zeros(ref.C, dtype=torch.float64)] * 3 if start is None else [None if s is None else s.double() for s in start]
    # (the start value is one more summand of the accumulation: it counts in the scale)
    eg = ((dgamma.double() - s0[0] - ref.dgamma).abs() - ref.flip_dgamma).clamp_min(0.0)
    eb = ((dbeta.double() - s0[1] - ref.dbeta).abs() - ref.flip_dbeta).clamp_min(0.0)
    out["dgamma"] = float((eg / (ref.abs_dgamma + s0[0].abs()).clamp_min(1e-300)).max())
    out["dbeta"] = float((eb / (ref.abs_dbeta + s0[1].abs()).clamp_min(1e-300)).max())
    if dxsum is not None:
        out["dxsum"] = float(((dxsum.double() - s0[2] - sum_dx).abs() / (abs_dx + s0[2].abs()).clamp_min(1e-300)).max())
    if eps is not None:
        assert out["dx"] <= eps, f"{what}: dx: {out['dx']:.3e} > {eps:.3e}"
    if eps_s is not None:
        for key in ("dgamma", "dbeta", "dxsum"):
            if key in out:
                assert out[key] <= eps_s, f"{what}: {key}: {out[key]:.3e} > {eps_s:.3e}"
    return out
