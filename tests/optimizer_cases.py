"""Host-side cases and references for the fused optimizer and loss scaler
(csrc/ngp_head.h adam_sweep / adam_sweep_pipe, csrc/ngp_step.h step_end_block,
csrc/nerf_fused.hip k_nonfinite, csrc/adam.hip). numpy only: no GPU, no torch.

  adam_reference_f64   torch.optim.Adam on g = float(g16) * grad_mult / scale, float64 (THE reference)
  adam_restated_f32    the kernels' own operation order in float32: the yardstick of the GPU margin only
  ScalerMachine        step_end_block restated over (scale, growth_tracker, adam_step, epoch, iter)
  SCHEDULE/TRAJECTORY  14 updates, growth_interval 3, iters 8, an inf in updates {2, 6, 7, 11}
  make_case            ragged tensor lists (R8, R4, R1, RBIG, EPS) inside canaried buffers
"""
import math

import numpy as np

LR, B1, B2, EPS = 1e-2, 0.9, 0.99, 1e-15
F32 = np.float32

# ---- the schedule ---------------------------------------------------------------------------------
SCHEDULE = dict(growth_interval=3, iters=8, K=14, init_scale=65536.0, inf_updates=(2, 6, 7, 11))
# (scale, growth tracker, Adam step, LR epoch) after each update: torch's own GradScaler("cpu",
# growth_interval=3) + Adam + LambdaLR(0.1 ** min(it / 8, 1)), asserted against torch in
# test_optimizer_cases_cpu.py
TRAJECTORY = [(65536, 1, 1, 1), (65536, 2, 2, 2), (32768, 0, 2, 3), (32768, 1, 3, 4), (32768, 2, 4, 5),
              (65536, 0, 5, 6), (32768, 0, 5, 7), (16384, 0, 5, 8), (16384, 1, 6, 9), (16384, 2, 7, 10),
              (32768, 0, 8, 11), (16384, 0, 8, 12), (16384, 1, 9, 13), (16384, 2, 10, 14)]


class ScalerMachine:
    """step_end_block's bookkeeping: GradScaler.update, the Adam step count,
    the LambdaLR epoch and the finished-step count. found_inf bit 0: an inf/nan
    (skip, back off, tracker reset); bit 1: the gradient exchange overflowed
    (skip only). The sweep's own part rides along: 1 / scale (x grad_mult) not
    finite in float32 sets bit 0, as GradScaler's unscale would find."""

    def __init__(self, scale=65536.0, growth_factor=2.0, backoff_factor=0.5, growth_interval=2000, enabled=True,
                 grad_mult=1.0):
        self.scale, self.tracker, self.adam_step, self.epoch, self.iter = F32(scale), 0, 0, 0, 0
        self.growth_factor, self.backoff_factor = F32(growth_factor), F32(backoff_factor)
        self.growth_interval, self.enabled, self.grad_mult = int(growth_interval), bool(enabled), F32(grad_mult)

    def unscale_overflows(self):
        with np.errstate(divide="ignore", over="ignore"):
            return not np.isfinite(F32(1.0 / np.float64(self.scale)) * self.grad_mult)

    def update(self, found_inf=0):
        """One update; -> whether Adam was skipped."""
        found_inf = int(found_inf) | int(self.unscale_overflows())
        skip, inf = found_inf != 0, (found_inf & 1) != 0
        if self.enabled:
            if inf:
                self.scale = F32(self.scale * self.backoff_factor)
                self.tracker = 0
            elif not skip:
                self.tracker += 1
                if self.tracker == self.growth_interval:
                    self.scale = F32(self.scale * self.growth_factor)
                    self.tracker = 0
        if not skip:
            self.adam_step += 1
        self.epoch += 1
        self.iter += 1
        return skip

    def state(self):
        return (float(self.scale), self.tracker, self.adam_step, self.epoch, self.iter)

    def lr(self, base_lr=LR, iters=8):
        return base_lr * 0.1 ** min(self.epoch / iters, 1)


def run_machine(found_inf_of=None, **kw):
    """The schedule through ScalerMachine -> [(scale, tracker, adam_step, epoch)] after each update."""
    s = SCHEDULE
    mach = ScalerMachine(s["init_scale"], growth_interval=s["growth_interval"], **kw)
    out = []
    for it in range(s["K"]):
        mach.update(int(it in s["inf_updates"]) if found_inf_of is None else found_inf_of(it))
        out.append(tuple(int(x) for x in mach.state()[:4]))
    return out


def trajectory_transitions(traj, init_scale=SCHEDULE["init_scale"], iters=SCHEDULE["iters"]):
    """What the schedule must contain, counted on a trajectory."""
    prev = [(int(init_scale), 0, 0, 0)] + list(traj[:-1])
    grow = [b[0] > a[0] for a, b in zip(prev, traj)]
    back = [b[0] < a[0] for a, b in zip(prev, traj)]
    return dict(
        inf_resets_tracker_of_2=sum(bk and a[1] == 2 for a, bk in zip(prev, back)),
        growths=sum(grow),
        growth_then_backoff=sum(g and b for g, b in zip(grow[:-1], back[1:])),
        backoffs_in_a_row=sum(a and b for a, b in zip(back[:-1], back[1:])),
        first_lag=next((i for i, t in enumerate(traj) if t[2] < t[3]), None),
        # updates that compute their LR at or past the clamp: the epoch BEFORE the update is >= iters
        clamped_updates=sum(a[3] >= iters for a in prev),
        applied=traj[-1][2])


# ---- Adam -----------------------------------------------------------------------------------------
def adam_reference_f64(p, m, v, g16, *, scale=1.0, grad_mult=1.0, step=1, lr=LR, betas=(B1, B2), eps=EPS,
                       weight_decay=0.0):
    """torch.optim.Adam (L2 weight decay) in float64, `step` the 1-based count
    of this update, lr the scheduled rate. g16: fp16 or fp32 gradients as stored.
    -> (p, m, v) float64, inputs untouched."""
    b1, b2 = betas
    p, m, v = (np.asarray(x, np.float64) for x in (p, m, v))
    g = np.asarray(g16).astype(np.float64) * np.float64(grad_mult) / np.float64(scale)
    if weight_decay != 0:
        g = g + weight_decay * p
    m = b1 * m + (1 - b1) * g
    v = b2 * v + (1 - b2) * g * g
    bc1, bc2 = 1 - b1 ** step, 1 - b2 ** step
    denom = np.sqrt(v) / math.sqrt(bc2) + eps
    return p - lr / bc1 * m / denom, m, v


def scheduled_lr(epoch, iters, base_lr=LR):
    return base_lr * 0.1 ** min(epoch / iters, 1)


def adam_restated_f32(p, m, v, g16, *, scale=1.0, grad_mult=1.0, adam_step=0, epoch=0, iters=30000, lr=LR,
                      betas=(B1, B2), eps=EPS):
    """adam_consts + adam_update (csrc/ngp_step.h) in the kernels' own float32
    operation order; adam_step / epoch are the state words BEFORE the update.
    -> (p, m, v) float32. A yardstick of the rounding to expect, not a reference."""
    b1, b2, eps, base_lr = F32(betas[0]), F32(betas[1]), F32(eps), F32(lr)
    inv_scale = F32(1.0 / np.float64(F32(scale))) * F32(grad_mult)
    step = adam_step + 1
    lr_t = np.float64(base_lr) * math.pow(0.1, min(epoch / iters, 1.0))
    bc1, bc2 = 1.0 - math.pow(np.float64(b1), step), 1.0 - math.pow(np.float64(b2), step)
    step_size = F32(lr_t / bc1)
    inv_bc2_sqrt = F32(1.0) / F32(math.sqrt(bc2))
    p, m, v = (np.asarray(x, F32) for x in (p, m, v))
    gk = np.asarray(g16).astype(F32) * inv_scale
    m = m + (F32(1.0) - b1) * (gk - m)
    v = v * b2 + (F32(1.0) - b2) * gk * gk
    denom = np.sqrt(v) * inv_bc2_sqrt + eps
    return p - step_size * (m / denom), m, v


def adam_step_restated_f32(p, m, v, g, *, lr=LR, betas=(B1, B2), eps=EPS, weight_decay=0.0, step=1,
                           grad_scale=1.0):
    """ngp_adam_step (csrc/adam.hip) in its own float32 operation order."""
    b1, b2, eps, wd, gs = F32(betas[0]), F32(betas[1]), F32(eps), F32(weight_decay), F32(grad_scale)
    bc1, bc2 = 1.0 - math.pow(np.float64(b1), step), 1.0 - math.pow(np.float64(b2), step)
    lr_bc1, inv_sqrt_bc2 = F32(np.float64(F32(lr)) / bc1), F32(1.0 / math.sqrt(bc2))
    p, m, v = (np.asarray(x, F32) for x in (p, m, v))
    gk = np.asarray(g).astype(F32) * gs
    if wd != 0:
        gk = gk + wd * p
    m = m + (F32(1.0) - b1) * (gk - m)
    v = v * b2 + (F32(1.0) - b2) * gk * gk
    denom = np.sqrt(v) * inv_sqrt_bc2 + eps
    return p - lr_bc1 * (m / denom), m, v


# ngp_adam_step's cases: (gradient dtype, weight decay, grad_scale, step, n)
ADAM_STEP_CASES = [(dt, wd, gs, step, n) for dt in ("f32", "f16") for wd in (0.0, 0.01)
                   for gs in (1.0, 1 / 65536) for step in (1, 2, 1000) for n in (1, 3, 4, 5, 1027)]


def adam_step_inputs(dt, gs, n, seed=0):
    rng = np.random.default_rng(seed + n)
    p = (rng.standard_normal(n) * 0.05).astype(np.float32)
    m = (rng.standard_normal(n) * 1e-3).astype(np.float32)
    v = (rng.random(n) * 1e-6 + 1e-9).astype(np.float32)
    g = rng.standard_normal(n) * 1e-3 / gs
    g = np.clip(g, -65000, 65000).astype(np.float16 if dt == "f16" else np.float32)
    return p, m, v, g


def ulp32(ref):
    """The float32 spacing at |ref| (float64 in, float64 out)."""
    return np.spacing(np.abs(np.asarray(ref, np.float64)).astype(F32)).astype(np.float64)


def error_figures(got, ref):
    """-> (max error in ulp32(|ref|), relative norm) of `got` against the float64 `ref`."""
    got, ref = np.asarray(got, np.float64).ravel(), np.asarray(ref, np.float64).ravel()
    if ref.size == 0:
        return 0.0, 0.0
    err = np.abs(got - ref)
    nrm = float(np.linalg.norm(ref))
    return float((err / ulp32(ref)).max()), (float(np.linalg.norm(err)) / nrm if nrm > 0 else float(err.max() > 0))


MARGIN = 4.0  # the device may err 4x the float32 restatement's own error (floor: 1 ulp32 of the reference)


def within_margin(got, ref, restated_figures):
    """The GPU tolerance of one tensor kind -> (ok, measured (max ulp, rel norm), allowed (max ulp, rel norm))."""
    mu, rn = error_figures(got, ref)
    amu, arn = max(MARGIN * restated_figures[0], 1.0), MARGIN * restated_figures[1]
    if np.asarray(ref).size and not np.isfinite(np.asarray(got, np.float64)).all():
        return False, (mu, rn), (amu, arn)
    # the per-value floor's counterpart: values within one ulp32 of the reference (up to 2^-23
    # relative each) cannot be held to a relative norm of 4 x 0
    arn = max(arn, 2.0 ** -23)
    return mu <= amu and rn <= arn, (mu, rn), (amu, arn)


# ---- ragged tensor lists -----------------------------------------------------------------------------
K_MAX_TENSORS = 8
PLAIN_CHUNK = 2048     # adam_sweep<2>: kAdamThreads * 4 * U
NONFINITE_CAP = 8192 * 256 * 8  # k_nonfinite's grid: values per trip of its grid-stride loop
SIZES = {
    "R8": [1, 3, 4, 5, 7, 8, 9, 2047],       # kMaxTensors; every chunk a seam, all but one tensor end in padding
    "R4": [2048, 2049, 6145, 12],            # a whole chunk | chunk + 1-element seam | 3 chunks + tail | short last
    "R1": [1],
    "RBIG": [NONFINITE_CAP + 2048 + 3],      # second trip of k_nonfinite's loop; past 16 x 256 CUs x 2048 too
    "EPS": [2048 + 260],                     # scale 2^24: the smallest fp16 subnormal beside eps
}
NULL_SHADOW = {"R8": (1, 4, 6), "R4": (1,), "R1": (), "RBIG": (), "EPS": (0,)}
MISALIGNED_GRAD = {"R8": 5, "R4": 2}         # this tensor's grad pointer is 8- but not 16-byte aligned
CASE_SCALE = {"EPS": 2.0 ** 24}
GUARD = 32                                   # canary elements before, between and behind the tensors
SENTINEL16 = 0x5555                          # the shadows' starting bits (a finite fp16)
_CANARY32 = {"p": 0x7fc0a001, "m": 0x7fc0a002, "v": 0x7fc0a003}
_CANARY16 = {"g": 0x7e11, "h": 0x7e22}
HALF_MAX, HALF_TINY_BITS = 65504.0, 0x0001   # the largest finite fp16, the smallest subnormal (2^-24)


def flat_starts(sizes):
    """make_list's flat index space: every tensor starts 8-aligned."""
    st = [0]
    for n in sizes:
        st.append(st[-1] + (n + 7) // 8 * 8)
    return st


def seam_masks(sizes, chunk=PLAIN_CHUNK):
    """Per tensor, which elements a sweep of `chunk` handles in its per-element
    seam loop (True) and which in whole 4-value groups (False)."""
    st = flat_starts(sizes)
    out = [np.ones(n, bool) for n in sizes]

    def find(i):
        k = 0
        while k + 1 < len(sizes) and i >= st[k + 1]:
            k += 1
        return k
    for c0 in range(0, st[-1], chunk):
        c1 = min(c0 + chunk, st[-1])
        k = find(c0)
        if find(c1 - 1) == k and c1 - st[k] <= sizes[k]:
            out[k][c0 - st[k]:c1 - st[k]] = False
    return out


class Case:
    """One tensor list. buf[kind] (p, m, v float32; g, h float16 as uint16 bits
    for g/h canaries' sake) holds every tensor of that kind between canaries;
    off[kind][k] is tensor k's first element in it, canary[kind] marks what no
    kernel may touch. packed: the gradients lie in one flat buffer the way
    make_list lays them out, the padding between them +0 (not canaries)."""

    def __init__(self, name, sizes, scale, packed):
        self.name, self.sizes, self.scale, self.packed = name, list(sizes), float(scale), packed
        self.buf, self.off, self.canary = {}, {}, {}
        self.null_shadow = tuple(NULL_SHADOW.get(name, ()))
        self.misaligned = None if packed else MISALIGNED_GRAD.get(name)
        self.padding = None  # packed: mask of the gradient buffer's alignment padding

    def n(self):
        return len(self.sizes)

    def view(self, kind, k, buf=None):
        b = self.buf[kind] if buf is None else buf
        return b[self.off[kind][k]:self.off[kind][k] + self.sizes[k]]

    def has_shadow(self, k):
        return k not in self.null_shadow

    def grad_byte_misaligned(self, k):
        return (self.off["g"][k] * 2) % 16 != 0  # the buffers themselves are allocated 16-byte aligned

    def nonfinite_path(self, k, off):
        """Which branch of k_nonfinite reads element `off` of tensor k."""
        tail = off // 8 * 8 + 8 > self.sizes[k]
        return "scalar" if tail or self.grad_byte_misaligned(k) else "vector"

    def flat_index(self, k, off):
        return flat_starts(self.sizes)[k] + off

    def groups(self):
        """Per tensor, which 4-value groups are idle for the sweep (m = v = +0 and g = +-0)."""
        out = []
        for k, n in enumerate(self.sizes):
            pad = (-n) % 4
            def g4(a, fill):
                return np.concatenate([a, np.full(pad, fill, a.dtype)]).reshape(-1, 4)
            m, v = g4(self.view("m", k), 0), g4(self.view("v", k), 0)
            g = g4(self.view("g", k), 0)
            out.append(((g & 0x7fff) == 0).all(1) & (m == 0).all(1) & (v == 0).all(1))
        return out


def _layout(case, kind):
    """Offsets of every tensor in the buffer of one kind and the buffer's length."""
    offs, at = [], GUARD
    for k, n in enumerate(case.sizes):
        at = (at + 15) // 16 * 16
        if kind == "g" and case.misaligned == k:
            at += 4  # 8 bytes: legal for a gradient, but not the 16 the vector branch of k_nonfinite needs
        offs.append(at)
        at += n + GUARD
    return offs, at


def _content(name, sizes, scale, seed):
    """p, m, v (float32) and g (fp16) of every tensor: normal draws of both
    signs, unscaled O(1e-3); 4-value groups cycling through idle (+0 grads),
    gradient only, moments only, idle with -0 grads, and both, so idle and
    moved groups alternate; the largest finite fp16 of either sign."""
    rng = np.random.default_rng(seed)
    out = []
    for k, n in enumerate(sizes):
        kind = ((np.arange(n) // 4) + k + 1) % 5  # 0 idle, 1 gradient only, 2 moments only, 3 idle (-0), 4 both
        draw = rng.standard_normal(n, dtype=F32)
        g = np.clip(draw * F32(1e-3 * scale), -65000, 65000).astype(np.float16)
        # some exact zeros inside moved groups too (a group moves as a whole)
        g[(np.arange(n) % 7 == 3)] = 0
        g = np.where((kind == 1) | (kind == 4), g, np.float16(0))
        g[kind == 3] = np.float16(-0.0)
        hasm = (kind == 2) | (kind == 4)
        m = np.where(hasm, rng.standard_normal(n, dtype=F32) * F32(1e-3), F32(0))
        v = np.where(hasm, rng.random(n, dtype=F32) * F32(1e-6) + F32(1e-9), F32(0))
        p = rng.standard_normal(n, dtype=F32) * F32(0.05)
        big = np.flatnonzero((kind == 1) | (kind == 4))
        if big.size >= 2 and name != "EPS":
            g[big[0]], g[big[-1]] = np.float16(HALF_MAX), np.float16(-HALF_MAX)
        if name == "EPS":
            # zero moments and the smallest fp16 subnormal at scale 2^24: |g| / scale = 2^-48 = 3.6e-15
            sel = np.flatnonzero(kind == 1)[:192]
            tiny = np.full(sel.size, HALF_TINY_BITS, np.uint16)
            tiny[1::2] |= 0x8000
            g.view(np.uint16)[sel] = tiny
        out.append((p.astype(F32), m.astype(F32), v.astype(F32), g))
    return out


def make_case(name, seed=0, packed=False):
    """The case `name` of SIZES: buffers with canaries, tensor offsets, content."""
    sizes = SIZES[name]
    case = Case(name, sizes, CASE_SCALE.get(name, 65536.0), packed)
    content = _content(name, sizes, case.scale, seed * 1000 + sum(sizes) % 997)
    for kind in "pmvgh":
        half = kind in "gh"
        if kind == "g" and packed:
            st = flat_starts(sizes)
            offs, total = [GUARD + s for s in st[:-1]], GUARD + st[-1] + GUARD
        else:
            offs, total = _layout(case, kind)
        if half:
            buf = np.full(total, _CANARY16[kind], np.uint16)
        else:
            buf = np.full(total, _CANARY32[kind], np.uint32).view(F32)
        can = np.ones(total, bool)
        if kind == "g" and packed:
            buf[GUARD:GUARD + st[-1]] = 0
            can[GUARD:GUARD + st[-1]] = False
            case.padding = np.zeros(total, bool)
            case.padding[GUARD:GUARD + st[-1]] = True
        for k, n in enumerate(sizes):
            src = {"p": 0, "m": 1, "v": 2, "g": 3}.get(kind)
            val = np.full(n, SENTINEL16, np.uint16) if kind == "h" else content[k][src]
            buf[offs[k]:offs[k] + n] = val.view(np.uint16) if half else val
            can[offs[k]:offs[k] + n] = False
            if case.padding is not None and kind == "g":
                case.padding[offs[k]:offs[k] + n] = False
        case.buf[kind], case.off[kind], case.canary[kind] = buf, offs, can
    return case


def fresh_grads(case, update, scale):
    """Update `update`'s gradient of every tensor (fp16 bits): fresh normal
    draws at `scale`, zeros at every 7th place, every tensor touched."""
    rng = np.random.default_rng(7919 * (update + 1) + len(case.sizes))
    out = []
    for n in case.sizes:
        g = np.clip(rng.standard_normal(n, dtype=F32) * F32(1e-3 * scale), -65000, 65000).astype(np.float16)
        g[np.arange(n) % 7 == 3] = 0
        out.append(g.view(np.uint16).copy())
    return out


NONFINITE16 = {"+inf": 0x7c00, "-inf": 0xfc00, "nan": 0x7e00}


def inf_candidates(case):
    """(tensor, element) places where the tests put an inf: the first and last
    element of every tensor, and an element inside the misaligned gradient."""
    out = []
    for k, n in enumerate(case.sizes):
        out += [(k, 0), (k, n - 1)]
    if case.misaligned is not None:
        out.append((case.misaligned, case.sizes[case.misaligned] // 2))
    return sorted(set(out))


def schedule_inf_place(case, update):
    """Where update `update` of the schedule carries its inf: another place each time."""
    c = inf_candidates(case)
    return c[(3 * update + 1) % len(c)]


# ---- the restatement's own error: the margin's yardstick -----------------------------------------------
def one_update(case, grad_mult=1.0, adam_step=0, epoch=0, iters=30000):
    """One update of every tensor from the case's state -> per tensor
    (reference (p, m, v) float64, restated (p, m, v) float32)."""
    out = []
    for k in range(case.n()):
        p, m, v = (case.view(x, k) for x in "pmv")
        g = case.view("g", k).view(np.float16)
        ref = adam_reference_f64(p, m, v, g, scale=case.scale, grad_mult=grad_mult, step=adam_step + 1,
                                 lr=scheduled_lr(epoch, iters))
        res = adam_restated_f32(p, m, v, g, scale=case.scale, grad_mult=grad_mult, adam_step=adam_step,
                                epoch=epoch, iters=iters)
        out.append((ref, res))
    return out


def figures_over_tensors(pairs):
    """[(ref pmv, got pmv)] per tensor -> {kind: (max ulp, rel norm)} over the whole list."""
    out = {}
    for i, kind in enumerate("pmv"):
        ref = np.concatenate([np.asarray(r[i], np.float64) for r, _ in pairs])
        got = np.concatenate([np.asarray(g[i], np.float64) for _, g in pairs])
        out[kind] = error_figures(got, ref)
    return out


def run_schedule(case, applied=None):
    """The schedule on `case` (fresh gradients each update, an inf where the
    schedule says): the float64 reference and the float32 restatement, each
    carried through with the machine's scale and its own step / epoch counts.
    -> (machine states after each update, per tensor (ref pmv f64, restated pmv f32))."""
    s = SCHEDULE
    mach = ScalerMachine(s["init_scale"], growth_interval=s["growth_interval"])
    ref = [tuple(np.asarray(case.view(x, k), np.float64) for x in "pmv") for k in range(case.n())]
    res = [tuple(np.asarray(case.view(x, k), F32) for x in "pmv") for k in range(case.n())]
    states = []
    for it in range(s["K"]):
        scale = float(mach.scale)
        grads = fresh_grads(case, it, scale)
        if it not in s["inf_updates"]:
            for k in range(case.n()):
                g = grads[k].view(np.float16)
                ref[k] = adam_reference_f64(*ref[k], g, scale=scale, step=mach.adam_step + 1,
                                            lr=scheduled_lr(mach.epoch, s["iters"]))
                res[k] = adam_restated_f32(*res[k], g, scale=scale, adam_step=mach.adam_step, epoch=mach.epoch,
                                           iters=s["iters"])
        mach.update(int(it in s["inf_updates"]))
        states.append(mach.state())
    return states, list(zip(ref, res))
