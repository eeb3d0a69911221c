"""The distortion regulariser restated in float64 numpy from its pairwise
definition (not from the O(n) prefix form the kernels and the reference's
EffDistLoss use), and the hand-built ray set of the GPU tests.

For one ray with steps delta_i, midpoints m_i and composite weights w_i:
    dist = sum_i sum_j w_i w_j |m_i - m_j| + 1/3 sum_i delta_i w_i^2
    d dist / d w_i = 2 sum_j w_j |m_i - m_j| + 2/3 delta_i w_i
and, with w_i = (1 - exp(-sigma_i delta_i)) T_i, T_i = prod_{k<i} exp(-sigma_k delta_k)
(d w_j / d sigma_j = delta_j Tafter_j, d w_i / d sigma_j = -delta_j w_i for i > j):
    d dist / d sigma_j = delta_j (g_j Tafter_j - sum_{i>j} g_i w_i)
The weights follow the serial composite's stop rule: the first sample after
which T < T_thresh is the last one with a weight (it is included)."""
import numpy as np

T_THRESH, SCALE, LO, HI = 1e-4, 65536.0, 0.2, 1.0


def weights_serial(sigma, delta, T_thresh=T_THRESH):
    """w [n] (0 past the stop), Tafter [n], the number of samples with a weight."""
    sigma, delta = np.asarray(sigma, np.float64), np.asarray(delta, np.float64)
    n = sigma.shape[0]
    w, Ta = np.zeros(n), np.zeros(n)
    T, used = 1.0, 0
    for i in range(n):
        a = 1.0 - np.exp(-sigma[i] * delta[i])
        w[i] = a * T
        T *= 1.0 - a
        Ta[i] = T
        used = i + 1
        if T < T_thresh:
            break
    return w, Ta, used


def dist_pairwise(w, m, delta):
    w, m, delta = (np.asarray(v, np.float64) for v in (w, m, delta))
    return float((w[:, None] * w[None, :] * np.abs(m[:, None] - m[None, :])).sum() + (delta * w * w).sum() / 3.0)


def dist_grad_w(w, m, delta):
    w, m, delta = (np.asarray(v, np.float64) for v in (w, m, delta))
    return 2.0 * (np.abs(m[:, None] - m[None, :]) * w[None, :]).sum(1) + (2.0 / 3.0) * delta * w


def ray_dist(sigma, deltas, T_thresh=T_THRESH):
    """One ray from its samples (sigma [n], deltas [n, 2]) -> dist, d dist / d sigma [n]."""
    sigma, deltas = np.asarray(sigma, np.float64), np.asarray(deltas, np.float64)
    n = sigma.shape[0]
    if n == 0:
        return 0.0, np.zeros(0)
    delta, m = deltas[:, 0], np.cumsum(deltas[:, 1])
    w, Ta, used = weights_serial(sigma, delta, T_thresh)
    g = dist_grad_w(w, m, delta)
    gw = g * w
    behind = gw[::-1].cumsum()[::-1] - gw  # sum_{i>j} g_i w_i
    ds = delta * (g * Ta - behind)
    ds[used:] = 0.0
    return dist_pairwise(w, m, delta), ds


def rays_dist(c):
    """The ray set's dist [N] by list position and d dist / d sigma [M]; rays
    without a composite (no samples, overflowing M) give 0 and zero rows."""
    dist, ds = np.zeros(c["N"]), np.zeros(c["M"])
    for n, (o, k) in enumerate(zip(c["offs"], c["counts"])):
        if c["valid"][n]:
            dist[n], ds[o:o + k] = ray_dist(c["sigma"][o:o + k], c["deltas"][o:o + k])
    return dist, ds


# 0: no samples; 1, 2: the shortest rays; 64/65 the wave boundary; 256/257 the
# boundary between the kept chunks (kLossPre = 4) and the reloaded ones; the
# 96-sample ray has sigma 1e9 at its sample 5 and stops there; the 80-sample
# ray overflows M
COUNTS = [0, 1, 2, 63, 64, 65, 128, 255, 256, 257, 320, 96, 80]


def ray_set():
    """tests/test_gpu_fused_depth.py::loss_case's construction on COUNTS, with
    the serial reference's composite (oracle, CPU) and depth targets of every
    kind. Each ray's sigma * delta sums to ~3, so no ray but the 96-sample one
    stops early (asserted), and its first midpoint is 0.3."""
    import oracle
    rng = np.random.default_rng(17)
    N = len(COUNTS)
    offs = np.concatenate([[0], np.cumsum(COUNTS)[:-1]]).astype(np.int64)
    M = int(offs[-1]) + 40  # the last ray's 80 rows do not fit
    index = rng.permutation(N)  # the ray index is not the list position
    rays = np.stack([index, offs, COUNTS], -1).astype(np.int32)
    d0 = rng.uniform(0.003, 0.006, M).astype(np.float32)
    d1 = rng.uniform(0.001, 0.003, M).astype(np.float32)
    sigma = np.zeros(M, np.float32)
    for o, k in zip(offs, COUNTS):
        e = min(o + k, M)
        if k:
            d1[o] = 0.3
            sigma[o:e] = rng.uniform(0.5, 1.5, e - o) * 3.0 / (k * 0.0045)
    stop_ray = COUNTS.index(96)
    sigma[offs[stop_ray] + 5] = 1e9
    deltas = np.stack([d0, d1], -1)
    valid = np.array([k > 0 and o + k <= M for o, k in zip(offs, COUNTS)])
    for n, (o, k) in enumerate(zip(offs, COUNTS)):
        if not valid[n]:
            continue
        used = weights_serial(sigma[o:o + k], d0[o:o + k])[2]
        sd = float((sigma[o:o + k].astype(np.float64) * d0[o:o + k]).sum())
        if n == stop_ray:
            assert used == 6
        else:  # exp(-8) = 3.4e-4 > T_thresh: the ray runs to its end
            assert used == k and 0.5 < sd < 8.0, (n, used, sd)
    col = rng.normal(0, 2, (M, 16)).astype(np.float16)
    h = rng.normal(0, 1, (M, 16)).astype(np.float16)
    gt = rng.uniform(0, 1, (N, 4)).astype(np.float32)
    bg = rng.uniform(0, 1, (N, 3)).astype(np.float32)
    rgbs = (1 / (1 + np.exp(-col[:, :3].astype(np.float32)))).astype(np.float16).astype(np.float32)
    ws, dp, img = oracle.composite_rays_train_forward(sigma, rgbs, deltas, rays, T_THRESH)
    pred = dp[index]  # by list position
    kinds = ["in", "above", "below", "low", "high", "zero", "nan"]
    kind = ["in" if not valid[n] else kinds[n % len(kinds)] for n in range(N)]
    val = {"in": 0.5, "low": 0.1, "high": 1.5, "zero": 0.0, "nan": np.nan}
    gtd_n = np.array([pred[n] + 0.25 if k == "above" else pred[n] - 0.05 if k == "below" else val[k]
                      for n, k in enumerate(kind)], np.float32)
    gtd = np.zeros(N, np.float32)
    gtd[index] = gtd_n  # the kernel reads the target by ray index
    c = dict(N=N, M=M, counts=COUNTS, rays=rays, index=index, offs=offs, sigma=sigma, deltas=deltas, col=col, h=h,
             gt=gt, bg=bg, rgbs=rgbs, ws=ws, dp=dp, img=img, gtd=gtd, valid=valid, stop_ray=stop_ray)
    c["dist"], c["dsigma"] = rays_dist(c)
    return c


def loss_reference(c, cw, dw, distw):
    """loss_ray, and the fp16 gradients the reference chain gives, as
    tests/test_gpu_fused_depth.py::_loss_reference forms them (the oracle's
    composite backward with grad_depth, rgbs.float() <- half and the sigmoid
    backward, sigmas = trunc_exp(h0) backward), with distw * dist in the loss
    and SCALE * distw / N * d dist / d sigma added to the density gradient
    before the trunc_exp backward and the rounding to half."""
    import oracle
    N, index = c["N"], c["index"]
    f32 = np.float32
    p = c["img"] + (1 - c["ws"])[:, None] * c["bg"]  # by ray index, as the reference's [N] tensors
    a = c["gt"][:, 3:]
    q = c["gt"][:, :3] * a + c["bg"] * (1 - a)
    e = (p - q).astype(f32)
    mse = ((e * e).sum(-1) / 3).astype(f32)
    pred = np.maximum(c["dp"], 0)
    with np.errstate(invalid="ignore"):
        mask = (LO <= c["gtd"]) & (c["gtd"] <= HI)
        dep = np.where(mask, np.abs(c["gtd"] - pred), 0).astype(f32)
        sgn = np.where(mask, np.sign(pred - c["gtd"]), 0).astype(f32)
    loss = (cw * mse + dw * dep).astype(np.float64)[index] + distw * c["dist"]
    g_img = (f32(SCALE * cw / N / 3) * 2 * e).astype(f32)
    g_ws = -(g_img * c["bg"]).sum(-1).astype(f32)
    g_dep = (f32(SCALE * dw / N) * sgn).astype(f32)
    gs, gc = oracle.composite_rays_train_backward(g_ws, g_dep, g_img, c["sigma"], c["rgbs"], c["deltas"], c["rays"],
                                                  c["ws"], c["dp"], c["img"], T_THRESH)
    gs = gs.astype(np.float64) + (SCALE * distw / N) * c["dsigma"]
    y = c["rgbs"]
    g_col = np.zeros((c["M"], 16), np.float16)
    with np.errstate(over="ignore"):
        g_col[:, :3] = (gc.astype(np.float16).astype(f32) * (1 - y) * y).astype(np.float16)
        g_h0 = (gs * np.exp(np.clip(c["h"][:, 0].astype(np.float64), -15, 15))).astype(np.float16)
    return loss, g_col, g_h0
