"""Float64 restatement of the normalisation / activation epilogue passes (csrc/elementwise.hip: snvc_norm_stats, snvc_affine_act,
snvc_act_backward_reduce / _apply, snvc_bn_backward_coefs, snvc_bn_track), written from the definitions of the operations: numpy
only, no GPU, nothing shared with the kernels.  Every function takes the float32 inputs a kernel would get and works in float64.

Layouts are those of snvc_amd.ops: tensors [N, C, *spatial]; per-channel vectors [C] or [1, C] (``per_sample=False``, train-mode
BatchNorm) or [N, C] (``per_sample=True``, GroupNorm); statistics [1, C] or [N, groups].

tests/test_epilogue_ref_host.py pins this file against float64 torch (F.batch_norm / F.group_norm and their autograd) on the CPU;
tests/test_gpu_epilogue.py holds the kernels to it."""
import numpy as np

# the epilogue flag bits of the C ABI (include/snvc_hip.h: SNVC_EPI_*)
EPI_RELU, EPI_ADD_PRE, EPI_ADD_POST, EPI_SIGMOID = 1, 2, 4, 8

U = 2.0 ** -24          # unit roundoff of float32 (round to nearest): |fl(a) - a| <= U * |a|


def f64(a):
    return None if a is None else np.asarray(a, dtype=np.float64)


def _vec(v, n, c, ndim, per_sample, default):
    """A per-channel or per-(n, c) vector (or None -> ``default``) as [N or 1, C, 1, ...] in float64."""
    tail = (1,) * (ndim - 2)
    if v is None:
        return np.full((1, c) + tail, default, dtype=np.float64)
    v = f64(v).reshape(-1, c)
    assert v.shape[0] == (n if per_sample else 1), (v.shape, n, per_sample)
    return v.reshape(v.shape + tail)


def _rows(x, groups, per_sample):
    """The statistics rows of x as [outer, groups, count]: (n, group) for GroupNorm, (channel over the batch) for BatchNorm."""
    x = f64(x)
    n, c = x.shape[:2]
    assert c % groups == 0
    if per_sample:
        return x.reshape(n, groups, -1)
    assert groups == c, "batch statistics are per channel"
    return np.moveaxis(x.reshape(n, c, -1), 0, 1).reshape(1, c, -1)


def norm_moments_ref(x, groups, per_sample):
    """(count, mean|x|, mean x^2) per statistics row, [outer, groups]: what the error bounds of the statistics are relative to."""
    r = _rows(x, groups, per_sample)
    return r.shape[2], np.abs(r).mean(axis=2), (r * r).mean(axis=2)


def norm_stats_ref(x, gamma, beta, groups, per_sample, eps):
    """(scale, shift, mean, var): mean and BIASED variance (two passes) per row, scale = gamma / sqrt(var + eps),
    shift = beta - mean * scale, per channel of the row's group.  scale / shift [outer, C], mean / var [outer, groups]."""
    r = _rows(x, groups, per_sample)
    c = np.shape(x)[1]
    cpg = c // groups
    mean = r.mean(axis=2)
    var = ((r - mean[..., None]) ** 2).mean(axis=2)
    rstd = 1.0 / np.sqrt(var + float(eps))
    ga = np.ones(c) if gamma is None else f64(gamma).reshape(c)
    be = np.zeros(c) if beta is None else f64(beta).reshape(c)
    mu_c, rstd_c = np.repeat(mean, cpg, axis=1), np.repeat(rstd, cpg, axis=1)
    scale = rstd_c * ga[None]
    return scale, be[None] - mu_c * scale, mean, var


def norm_stats_bounds(x, gamma, groups, per_sample, eps):
    """(em, ev, b_scale, b_shift): how far statistics summed in float64 from the first element on, in any order, may lie from
    norm_stats_ref -- without the float32 storage terms (u |ref|), which the caller adds.  Each of the two sums (x and x^2 over a
    row of `count` elements) is off by at most count * 2^-53 * sum|terms|, one rounding per addition of partial sums that the sum of
    the magnitudes bounds:
        em = count * 2^-53 * mean|x|,     ev = 4 * count * 2^-53 * mean x^2     (var = E x^2 - mean^2, mean|x|^2 <= mean x^2),
    [outer, groups]; scale = gamma rstd and shift = beta - mean rstd gamma are formed in float64 from the unrounded mean / var: with
    rstd' = d rstd / d var = rstd^3 / 2 taken at the lowest admissible variance (where it is largest),
        b_scale = |gamma| ev rstd',       b_shift = |gamma| (em rstd + |mean| ev rstd' + em ev rstd'),   [outer, C]."""
    count, m_abs, m_sq = norm_moments_ref(x, groups, per_sample)
    _, _, r_mean, r_var = norm_stats_ref(x, gamma, None, groups, per_sample, eps)
    em, ev = count * 2.0 ** -53 * m_abs, 4 * count * 2.0 ** -53 * m_sq
    c = np.shape(x)[1]
    cpg = c // groups
    rep = lambda a: np.repeat(a, cpg, axis=1)       # noqa: E731
    ga = np.ones(c) if gamma is None else f64(gamma).reshape(c)
    rstd = 1.0 / np.sqrt(r_var + float(eps))
    d_rstd = 0.5 * (np.maximum(r_var - ev, 0.0) + float(eps)) ** -1.5 * ev
    b_scale = np.abs(ga)[None] * rep(d_rstd)
    b_shift = np.abs(ga)[None] * rep(em * rstd + np.abs(r_mean) * d_rstd + em * d_rstd)
    return em, ev, b_scale, b_shift


def preact_ref(x, scale, shift, res, flags, per_sample):
    """v, the argument of the activation: x * scale + shift, plus the residual under EPI_ADD_PRE; also the two affine terms."""
    x = f64(x)
    n, c = x.shape[:2]
    sc = _vec(scale, n, c, x.ndim, per_sample, 1.0)
    sh = _vec(shift, n, c, x.ndim, per_sample, 0.0)
    xs = x * sc
    v = xs + sh
    if flags & EPI_ADD_PRE:
        v = v + f64(res)
    return v, xs, np.broadcast_to(sh, x.shape)


def _act(v, flags):
    if flags & EPI_RELU:
        v = np.where(v > 0.0, v, 0.0)
    if flags & EPI_SIGMOID:
        v = 1.0 / (1.0 + np.exp(-v))
    return v


def affine_act_ref(x, scale, shift, res, flags, per_sample):
    """y = act(x * scale + shift [+ res]) [+ res] and the magnitude M = |x * scale| + |shift| + |res| + |y| that bounds every
    intermediate of a float32 evaluation (the residual counts only where a flag uses it)."""
    v, xs, sh = preact_ref(x, scale, shift, res, flags, per_sample)
    y = _act(v, flags)
    if flags & EPI_ADD_POST:
        y = y + f64(res)
    m = np.abs(xs) + np.abs(sh) + np.abs(y)
    if flags & (EPI_ADD_PRE | EPI_ADD_POST):
        m = m + np.abs(f64(res))
    return y, m


def act_grad_ref(raw, gy, res, scale, shift, flags, per_sample):
    """g = dL/dv = gy * act'(v); the ReLU derivative is 0 at v <= 0.  EPI_ADD_POST does not enter (the residual's own gradient is gy)."""
    v, _, _ = preact_ref(raw, scale, shift, res, flags, per_sample)
    g = f64(gy)
    if flags & EPI_RELU:
        g = np.where(v > 0.0, g, 0.0)
    if flags & EPI_SIGMOID:
        s = 1.0 / (1.0 + np.exp(-v))
        g = g * (s * (1.0 - s))
    return g


def act_backward_sums_ref(raw, g):
    """([sum g, sum g * raw], [sum |g|, sum |g * raw|]) per (n, c): [N, C, 2] each."""
    raw, g = f64(raw), f64(g)
    n, c = raw.shape[:2]
    a, b = g.reshape(n, c, -1), (g * raw).reshape(n, c, -1)
    return np.stack([a.sum(2), b.sum(2)], axis=2), np.stack([np.abs(a).sum(2), np.abs(b).sum(2)], axis=2)


def act_backward_apply_ref(raw, g, coef_g, coef_raw, coef_const, per_sample):
    """draw = A * g + B * raw + Cc with the coefficients indexed [c] or [n * C + c] (None: B = 0, Cc = 0), and the magnitude
    M = |A g| + |B raw| + |Cc| + |draw|."""
    raw, g = f64(raw), f64(g)
    n, c = raw.shape[:2]
    a = _vec(coef_g, n, c, raw.ndim, per_sample, 1.0)
    b = _vec(coef_raw, n, c, raw.ndim, per_sample, 0.0)
    cc = _vec(coef_const, n, c, raw.ndim, per_sample, 0.0)
    draw = a * g + b * raw + cc
    return draw, np.abs(a * g) + np.abs(b * raw) + np.abs(cc) + np.abs(draw)


def bn_backward_coefs_ref(sums, mean, var, gamma, count, eps):
    """Train-mode BatchNorm backward in closed form.  With xhat = (raw - mean) * rstd and y = gamma * xhat + beta:
        dbeta = sum g,   dgamma = sum g * xhat = rstd * (sum g raw - mean * sum g),
        draw  = gamma * rstd * (g - dbeta / count - xhat * dgamma / count) = coef_g * g + coef_raw * raw + coef_const.
    ``sums`` [N, C, 2] as act_backward_sums_ref, mean / var [C].  Returns (values, magnitudes): dicts of [C] vectors under the keys
    coef_g, coef_raw, coef_const, dgamma, dbeta; a magnitude is the sum of the absolute values of the terms of its expression."""
    sums, mu, var = f64(sums), f64(mean).reshape(-1), f64(var).reshape(-1)
    c = mu.shape[0]
    gam = np.ones(c) if gamma is None else f64(gamma).reshape(c)
    rstd = 1.0 / np.sqrt(var + float(eps))
    sg, sgr = sums[..., 0].sum(0), sums[..., 1].sum(0)
    sg_m, sgr_m = np.abs(sums[..., 0]).sum(0), np.abs(sums[..., 1]).sum(0)
    dgamma, dgamma_m = rstd * (sgr - mu * sg), rstd * (sgr_m + np.abs(mu) * sg_m)
    a = gam * rstd
    b, b_m = -a * rstd * dgamma / count, np.abs(a) * rstd * dgamma_m / count
    cc, cc_m = -a * sg / count - b * mu, np.abs(a) * sg_m / count + b_m * np.abs(mu)
    return (dict(coef_g=a, coef_raw=b, coef_const=cc, dgamma=dgamma, dbeta=sg),
            dict(coef_g=np.abs(a), coef_raw=b_m, coef_const=cc_m, dgamma=dgamma_m, dbeta=sg_m))


def gn_backward_coefs_ref(sums, mean, var, gamma, groups, count, eps):
    """The GroupNorm backward coefficients, the algebra of snvc_amd/models/submodule.py::_backward_coefs restated: statistics per
    (n, group) over ``count`` = cpg * S elements, sums per (n, c):
        sgx = rstd * (sgr - mu * sg);  p1 = sum_{c in group} gamma sg;  p2 = sum_{c in group} gamma sgx;
        A = rstd * gamma;  B = -rstd^2 * p2 / count;  Cc = -rstd * p1 / count - B * mu   (all [N, C]);
        dgamma = sum_n sgx, dbeta = sum_n sg.
    Returns (values, magnitudes) as bn_backward_coefs_ref."""
    sums, mean, var = f64(sums), f64(mean), f64(var)
    n, c = sums.shape[:2]
    cpg = c // groups
    gam = np.ones(c) if gamma is None else f64(gamma).reshape(c)
    mu, rstd = np.repeat(mean, cpg, axis=1), np.repeat(1.0 / np.sqrt(var + float(eps)), cpg, axis=1)
    sg, sgr = sums[..., 0], sums[..., 1]
    sgx, sgx_m = rstd * (sgr - mu * sg), rstd * (np.abs(sgr) + np.abs(mu * sg))

    def over_group(t):
        return np.repeat(t.reshape(n, groups, cpg).sum(2), cpg, axis=1)

    p1, p1_m = over_group(gam * sg), over_group(np.abs(gam * sg))
    p2, p2_m = over_group(gam * sgx), over_group(np.abs(gam) * sgx_m)
    a = rstd * gam
    b, b_m = -rstd * rstd * p2 / count, rstd * rstd * p2_m / count
    cc, cc_m = -rstd * p1 / count - b * mu, rstd * p1_m / count + b_m * np.abs(mu)
    return (dict(coef_g=a, coef_raw=b, coef_const=cc, dgamma=sgx.sum(0), dbeta=sg.sum(0)),
            dict(coef_g=np.abs(a), coef_raw=b_m, coef_const=cc_m, dgamma=sgx_m.sum(0), dbeta=np.abs(sg).sum(0)))


def frozen_bn_backward_coefs_ref(sums, running_mean, running_var, gamma, eps):
    """Eval-mode (frozen) BatchNorm backward: the statistics are constants, so draw = A * g with A = gamma * rstd of the RUNNING
    statistics and B = Cc = None; dgamma = rstd * (sum g raw - mean * sum g), dbeta = sum g.  Returns (values, magnitudes) as
    bn_backward_coefs_ref."""
    sums, mu, var = f64(sums), f64(running_mean).reshape(-1), f64(running_var).reshape(-1)
    c = mu.shape[0]
    gam = np.ones(c) if gamma is None else f64(gamma).reshape(c)
    rstd = 1.0 / np.sqrt(var + float(eps))
    sg, sgr = sums[..., 0].sum(0), sums[..., 1].sum(0)
    sg_m, sgr_m = np.abs(sums[..., 0]).sum(0), np.abs(sums[..., 1]).sum(0)
    a = gam * rstd
    return (dict(coef_g=a, coef_raw=None, coef_const=None, dgamma=rstd * (sgr - mu * sg), dbeta=sg),
            dict(coef_g=np.abs(a), coef_raw=None, coef_const=None, dgamma=rstd * (sgr_m + np.abs(mu) * sg_m), dbeta=sg_m))


def bn_track_ref(running_mean, running_var, num_batches_tracked, mean, var, count, momentum):
    """nn.BatchNorm's train-mode bookkeeping: running <- running + momentum * (batch - running), the batch variance made unbiased
    first (count / (count - 1); a single element has no unbiased variance and keeps the biased one), the counter + 1.
    Returns (running_mean, running_var, num_batches_tracked, magnitudes of the two updates = |running| + |batch|)."""
    rm, rv, mu = f64(running_mean), f64(running_var), f64(mean)
    ub = f64(var) * (float(count) / max(float(count) - 1.0, 1.0))
    return (rm + momentum * (mu - rm), rv + momentum * (ub - rv), int(num_batches_tracked) + 1,
            (np.abs(rm) + np.abs(mu), np.abs(rv) + np.abs(ub)))


def chain_ref(x, res, gy, gamma, beta, groups, per_sample, flags, eps):
    """y = act(norm(x) [+ res]) [+ res] and its backward for the upstream gradient gy, in the order the product runs the passes:
    norm_stats_ref -> affine_act_ref, then act_grad_ref -> act_backward_sums_ref -> coefficients -> act_backward_apply_ref.
    Returns a dict: y, draw, dgamma, dbeta, dres (the residual's gradient) and everything in between."""
    n, c = x.shape[:2]
    s = int(np.prod(x.shape[2:]))
    use_res = res if flags & (EPI_ADD_PRE | EPI_ADD_POST) else None
    scale, shift, mean, var = norm_stats_ref(x, gamma, beta, groups, per_sample, eps)
    y, m_y = affine_act_ref(x, scale, shift, use_res, flags, per_sample)
    g = act_grad_ref(x, gy, use_res, scale, shift, flags, per_sample)
    sums, sums_abs = act_backward_sums_ref(x, g)
    if per_sample:
        co, co_m = gn_backward_coefs_ref(sums, mean, var, gamma, groups, (c // groups) * s, eps)
    else:
        co, co_m = bn_backward_coefs_ref(sums, mean[0], var[0], gamma, n * s, eps)
    draw, m_draw = act_backward_apply_ref(x, g, co["coef_g"], co["coef_raw"], co["coef_const"], per_sample)
    dres = g if flags & EPI_ADD_PRE else (f64(gy) if flags & EPI_ADD_POST else np.zeros(x.shape))
    return dict(y=y, draw=draw, dgamma=co["dgamma"], dbeta=co["dbeta"], dres=dres, g=g, scale=scale, shift=shift, mean=mean, var=var,
                sums=sums, sums_abs=sums_abs, coefs=co, coef_mags=co_m, m_y=m_y, m_draw=m_draw)


def relu_edge(v, m):
    """Elements whose pre-activation is nearer to zero than 8 float32 roundings of the magnitude: a float32 evaluation may land on the
    other side of the ReLU there.  v == 0 with m == 0 (all terms exactly zero) is exact on both sides and is not an edge."""
    return (np.abs(v) < 8.0 * U * m) & (m > 0.0)


def clear_relu_edges(raw, scale, shift, res, flags, per_sample):
    """Move every element of ``raw`` (float32, changed in place) whose pre-activation is a ReLU edge (relu_edge) away from zero by 64
    roundings of its magnitude.  ``res`` enters v only under EPI_ADD_PRE, the magnitude whenever it is given.  Returns the number of elements moved; the caller asserts afterwards that none remains."""
    moved = 0
    for _ in range(8):
        v, xs, sh = preact_ref(raw, scale, shift, res, flags, per_sample)
        m = np.abs(xs) + np.abs(sh) + np.abs(v) + (np.abs(f64(res)) if res is not None else 0.0)     # >= M of every flag set with this v
        bad = relu_edge(v, m)
        if not bad.any():
            break
        n, c = raw.shape[:2]
        sc = np.broadcast_to(_vec(scale, n, c, raw.ndim, per_sample, 1.0), raw.shape)[bad]
        step = 64.0 * U * m[bad] / np.abs(sc) * np.where(v[bad] >= 0.0, 1.0, -1.0) * np.sign(sc)
        raw[bad] = (f64(raw[bad]) + step).astype(np.float32)
        moved += int(bad.sum())
    return moved
