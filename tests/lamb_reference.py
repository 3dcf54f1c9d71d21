"""fp64 reference of the LAMB step (csrc/optim.hip ia_lamb_flat; the definition is in DESIGN.md "LAMB" and include/itemalign.h), in
plain numpy with no call into the HIP library: one function per quantity (s, m, v, u, r_T, w), then `reference_step` over a test arena.

Hyper-parameters enter as the fp32 values the C ABI receives (`f32`): 1 - float32(0.999) differs from 0.001 by 3e-5 of itself, so a
reference fed the Python doubles would measure the ABI's argument types, not the kernels.

The per-element bars are derived here from the fp32 unit roundoff U = 2^-24 and the roundings the kernels perform (gamma(k) = kU / (1 - kU)
bounds k successive roundings).  Every step is judged on its own: the reference starts from the fp32 state (w, m, v) the step under test
started from, so no bar has to carry an earlier step's error.

  s     clipped only: each chunk's sum of g^2 is an fp32 chain of at most CHAIN = 24 roundings of non-negative terms (16 fused
        multiply-adds per thread, 6 levels of the wave tree, 2 of the workgroup; the squares are exact inside the fma), the chunks are
        added and the root taken in fp64, one rounding to fp32:  |ds| <= (gamma(CHAIN) / 2 + U) s = CS U s, CS = 13.  Unclipped: exact.
  m     g' = fl(g s); m = fma(b1, m, fl((1 - b1) g')), 1 - b1 exact:  |dm| <= gamma(1) |m| + gamma(2 + CS) (1 - b1) |g'|
  v     fl(g' g'), fl((1 - b2) .), fma:                               |dv| <= gamma(1) v + gamma(4 + 2 CS) (1 - b2) g'^2
  u     fl(m rbc1) (rbc1 itself one rounding), fl(v rbc2), sqrt, + eps, divide: 6 roundings on the quotient q, which also inherits
        dm and dv; then u = fma(wd, w, q):
        |dq| <= dm rbc1 / den + |q| (dv / (2 v) + gamma(6)),  |du| <= |dq| + gamma(1) |u|
  r_T   each norm: an fp32 chain per chunk as for s (relative gamma(CHAIN) / 2 on the norm), fp64 across chunks; |u| also moves by at most
        |du|_2 (triangle inequality); the quotient is fp64, rounded once:
        |dr| / r <= (1 + gamma(CHAIN) / 2) (1 + U) / (1 - gamma(CHAIN) / 2 - |du|_2 / |u|_2) - 1
  w     fl(lr r), then fma(-lr r, u, w):   |dw| <= lr r (|u| (dr / r + gamma(1)) + |du|) + gamma(1) |w_new|
  shadow = bf16 round-to-nearest-even of the fp32 w, bit for bit.
Where a gradient is not zero, the three roundings of m and of v may each land in the subnormal range (a real model has gradients of
1e-20), where a rounding moves a value by up to DENORM = 2^-149 whatever its size: 3 DENORM is added to dm and dv there.
"""
import numpy as np

U = 2.0 ** -24
CHAIN = 24
CS = 13
DENORM = 2.0 ** -149
CHUNK = 4096
ALIGN = 64
F64 = np.float64


def gamma(k):
    return k * U / (1.0 - k * U)


def f32(x):
    """a hyper-parameter as the kernels see it"""
    return float(np.float32(x))


class Hyper:
    def __init__(self, lr, b1=0.9, b2=0.999, eps=1e-6, wd=0.01, grad_scale=1.0, max_grad_norm=0.0):
        self.lr, self.b1, self.b2, self.eps, self.wd = f32(lr), f32(b1), f32(b2), f32(eps), f32(wd)
        self.grad_scale, self.max_grad_norm = f32(grad_scale), f32(max_grad_norm)

    def args(self):
        """(lr, beta1, beta2, eps, weight_decay) in ia_lamb_flat's order"""
        return self.lr, self.b1, self.b2, self.eps, self.wd


# ------------------------------------------------------------------------------------------------------------ the definition, fp64
def grad_factor(grads, grad_scale, max_grad_norm):
    """s: grads = the gradients of all trainable tensors"""
    if max_grad_norm <= 0:
        return grad_scale
    norm = np.sqrt(sum(float(np.sum(g.astype(F64) ** 2)) for g in grads))
    return grad_scale * min(1.0, max_grad_norm / (grad_scale * norm + 1e-6))


def first_moment(m, g, s, b1):
    return b1 * m.astype(F64) + (1.0 - b1) * (s * g.astype(F64))


def second_moment(v, g, s, b2):
    return b2 * v.astype(F64) + (1.0 - b2) * (s * g.astype(F64)) ** 2


def direction(m, v, w, b1, b2, eps, wd, t):
    """u from the NEW moments and the weights before the update; wd = 0 for a tensor that does not decay"""
    return (m / (1.0 - b1 ** t)) / (np.sqrt(v / (1.0 - b2 ** t)) + eps) + wd * w.astype(F64)


def trust_ratio(w, u, adapt):
    wn, un = np.sqrt(np.sum(w.astype(F64) ** 2)), np.sqrt(np.sum(u ** 2))
    return float(wn / un) if adapt and wn > 0 and un > 0 else 1.0


def new_weights(w, u, r, lr):
    return w.astype(F64) - lr * r * u


def bf16_bits(x32):
    """bf16 round-to-nearest-even of finite fp32 values, as uint16 bit patterns"""
    b = np.ascontiguousarray(x32, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return ((b + 0x7FFF + ((b >> 16) & 1)) >> 16).astype(np.uint16)


# ------------------------------------------------------------------------------------------------------------ the test arena
class Tensor:
    def __init__(self, name, n, flag, zero_g=False, zero_w=False, frozen=False):
        self.name, self.n, self.decay, self.adapt, self.zero_g, self.zero_w, self.frozen = name, n, flag, flag, zero_g, zero_w, frozen
        self.off = None

    @property
    def sl(self):
        return slice(self.off, self.off + self.n)


def arena_tensors(big=1 << 20):
    """1, 3, 63, 64, 65, 4095, 4096, 4097, 3 * 4096 + 5 and 2^20 elements; flags mixed; one tensor without gradient, one without weights,
    one frozen (in the arena, in no table)"""
    return [Tensor("a.weight", 1, True), Tensor("a.bias", 3, False), Tensor("zero_w.weight", 63, True, zero_w=True),
            Tensor("b.bias", 64, False), Tensor("zero_g.weight", 65, True, zero_g=True), Tensor("c.weight", 4095, True),
            Tensor("frozen.weight", 100, True, frozen=True), Tensor("c.LayerNorm.weight", 4096, False), Tensor("d.weight", 4097, True),
            Tensor("e.weight", 3 * 4096 + 5, True), Tensor("big.weight", big, True), Tensor("tail.bias", 130, False)]


class Arena:
    """Five flat buffers with ParamArena's layout (tensors at 64-element offsets).  Everything outside the tensors is NaN in all five."""

    def __init__(self, tensors, seed=0):
        rng = np.random.default_rng(seed)
        off = 0
        for t in tensors:
            t.off = off
            off += (t.n + ALIGN - 1) // ALIGN * ALIGN
        self.tensors, self.numel, self.rng = tensors, off + ALIGN, rng          # one more block of padding behind the last tensor
        self.w, self.g, self.m, self.v = (np.full(self.numel, np.nan, np.float32) for _ in range(4))
        self.shadow = np.full(self.numel, 0x7FC0, np.uint16)                        # bf16 NaN
        for t in tensors:
            self.w[t.sl] = 0.0 if t.zero_w else rng.normal(0.0, 0.05, t.n).astype(np.float32)
            self.m[t.sl] = 0.0
            self.v[t.sl] = 0.0
            self.shadow[t.sl] = bf16_bits(self.w[t.sl])
        self.new_grads()

    def new_grads(self):
        """|g| in [1e-3, 1e-1) with a random sign, or exactly 0 (one element in twenty): eps never decides a quotient"""
        for t in self.tensors:
            mag = 10.0 ** self.rng.uniform(-3.0, -1.0, t.n)
            g = mag * self.rng.choice([-1.0, 1.0], t.n) * (self.rng.random(t.n) >= 0.05)
            self.g[t.sl] = 0.0 if t.zero_g else g.astype(np.float32)
            a = np.abs(self.g[t.sl])
            assert ((a == 0) | (a >= np.float32(1e-3))).all()

    @property
    def trainable(self):
        return [t for t in self.tensors if not t.frozen]

    def tables(self):
        """(chunk table [n_chunks, 4] uint32, tensor table [n_tensors, 3] uint32) of ia_lamb_flat over the trainable tensors"""
        chunks, tens = [], []
        for t in self.trainable:
            tens.append((len(chunks), (t.n + CHUNK - 1) // CHUNK, 1 if t.adapt else 0))
            for c in range(0, t.n, CHUNK):
                chunks.append(((t.off + c) & 0xFFFFFFFF, (t.off + c) >> 32, min(CHUNK, t.n - c), 1 if t.decay else 0))
        return np.asarray(chunks, np.uint32).reshape(-1, 4), np.asarray(tens, np.uint32).reshape(-1, 3)

    def padding_mask(self):
        """True where no trainable tensor lives: alignment padding and the frozen tensor"""
        mask = np.ones(self.numel, bool)
        for t in self.trainable:
            mask[t.sl] = False
        return mask


# ------------------------------------------------------------------------------------------------------------ one step + its bars
class Expected:
    """per tensor name: fp64 m, v, u, w and r with the bars dm, dv, du, dw (arrays) and dr (a number)"""


def reference_step(tensors, w, g, m, v, hp, t):
    """The step `t` from the fp32 state (w, m, v) and gradients g (flat arrays), over `tensors` (each with .sl, .decay, .adapt).
    -> (s, {name: Expected})"""
    clipped = hp.max_grad_norm > 0
    s = grad_factor([g[x.sl] for x in tensors], hp.grad_scale, hp.max_grad_norm)
    cs = CS if clipped else 0
    rbc1, rbc2 = 1.0 / (1.0 - hp.b1 ** t), 1.0 / (1.0 - hp.b2 ** t)
    out = {}
    for x in tensors:
        e = Expected()
        wd = hp.wd if x.decay else 0.0
        w0, gp = w[x.sl].astype(F64), s * g[x.sl].astype(F64)
        e.m = first_moment(m[x.sl], g[x.sl], s, hp.b1)
        e.v = second_moment(v[x.sl], g[x.sl], s, hp.b2)
        e.dm = gamma(1) * np.abs(e.m) + gamma(2 + cs) * (1.0 - hp.b1) * np.abs(gp) + 3 * DENORM * (gp != 0)
        e.dv = gamma(1) * e.v + gamma(4 + 2 * cs) * (1.0 - hp.b2) * gp ** 2 + 3 * DENORM * (gp != 0)
        e.u = direction(e.m, e.v, w[x.sl], hp.b1, hp.b2, hp.eps, wd, t)
        den = np.sqrt(e.v * rbc2) + hp.eps
        q = e.m * rbc1 / den
        rel_v = np.divide(e.dv, 2.0 * e.v, out=np.zeros_like(e.v), where=e.v > 0)
        e.du = e.dm * rbc1 / den + np.abs(q) * (rel_v + gamma(6)) + gamma(1) * np.abs(e.u)
        e.r = trust_ratio(w[x.sl], e.u, x.adapt)
        un = np.sqrt(np.sum(e.u ** 2))
        if x.adapt and un > 0 and np.any(w0 != 0):
            rel_u = float(np.sqrt(np.sum(e.du ** 2)) / un)
            rel_r = (1.0 + gamma(CHAIN) / 2) * (1.0 + U) / (1.0 - gamma(CHAIN) / 2 - rel_u) - 1.0
        else:
            rel_r = 0.0                      # r = 1 by definition: exact
        e.dr = rel_r * e.r
        e.w = new_weights(w[x.sl], e.u, e.r, hp.lr)
        e.dw = hp.lr * e.r * (np.abs(e.u) * (rel_r + gamma(1)) + e.du) + gamma(1) * np.abs(e.w)
        out[x.name] = e
    return s, out


# ------------------------------------------------------------------------------------------------------------ fp32 model of the kernels
def _fma(a, b, c):
    """fused multiply-add of fp32 values: the product of two fp32 numbers is exact in fp64"""
    return (np.asarray(a, np.float32).astype(F64) * np.asarray(b, np.float32).astype(F64) + np.asarray(c, np.float32).astype(F64)).astype(np.float32)


def _chunk_sumsq(x32):
    """one chunk's sum of squares in fp32 (pairwise: no chain longer than the kernels')"""
    return np.sum(x32.astype(np.float32) ** 2, dtype=np.float32)


def kernel_model_step(tensors, w, g, m, v, hp, t, fault=None):
    """What the kernels compute, in numpy fp32: fp32 partial sums per chunk, fp64 across chunks.  Returns new (w, m, v, shadow bits,
    {name: r}); the inputs are not modified.  fault: None, or one of "ratio_per_chunk", "padding_in_norm", "no_bias_correction" --
    the three mistakes the bars must catch."""
    f = np.float32
    w, m, v = w.copy(), m.copy(), v.copy()
    shadow = np.zeros(len(w), np.uint16)
    if hp.max_grad_norm > 0:
        total = sum(float(_chunk_sumsq(g[x.off + c:x.off + min(c + CHUNK, x.n)])) for x in tensors for c in range(0, x.n, CHUNK))
        s = f(hp.grad_scale * min(1.0, hp.max_grad_norm / (np.sqrt(total) * hp.grad_scale + 1e-6)))
    else:
        s = f(hp.grad_scale)
    b1, b2, eps, lr = f(hp.b1), f(hp.b2), f(hp.eps), f(hp.lr)
    if fault == "no_bias_correction":
        rbc1 = rbc2 = f(1.0)
    else:
        rbc1, rbc2 = f(1.0 / (1.0 - hp.b1 ** t)), f(1.0 / (1.0 - hp.b2 ** t))
    ratios = {}
    for x in tensors:
        wd = f(hp.wd if x.decay else 0.0)
        gr = g[x.sl] * s
        m[x.sl] = _fma(b1, m[x.sl], (f(1) - b1) * gr)
        v[x.sl] = _fma(b2, v[x.sl], (f(1) - b2) * (gr * gr))
        u = _fma(wd, w[x.sl], (m[x.sl] * rbc1) / (np.sqrt(v[x.sl] * rbc2) + eps))
        spans = [(c, min(c + CHUNK, x.n)) for c in range(0, x.n, CHUNK)]
        pw = [float(_chunk_sumsq(w[x.off + a:x.off + b])) for a, b in spans]
        pu = [float(_chunk_sumsq(u[a:b])) for a, b in spans]
        if fault == "padding_in_norm":      # the alignment padding read as weights (finite stand-ins: the real padding is NaN)
            pw[-1] += float(((x.off + x.n + ALIGN - 1) // ALIGN * ALIGN - (x.off + x.n)) * 0.05 ** 2)

        def ratio(sw, su):
            return f(np.sqrt(sw) / np.sqrt(su)) if x.adapt and sw > 0 and su > 0 else f(1.0)
        r = ratio(sum(pw), sum(pu))
        ratios[x.name] = float(r)
        for i, (a, b) in enumerate(spans):
            rc = ratio(pw[i], pu[i]) if fault == "ratio_per_chunk" else r
            w[x.off + a:x.off + b] = _fma(-(lr * rc), u[a:b], w[x.off + a:x.off + b])
        shadow[x.sl] = bf16_bits(w[x.sl])
    return w, m, v, shadow, ratios


def worst(got, want, bar):
    """largest |got - want| / bar over the elements (0 where the bar is 0 and the value exact; inf where it is not)"""
    err = np.abs(np.asarray(got, F64) - want)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(bar > 0, err / bar, np.where(err == 0, 0.0, np.inf))
    return float(np.max(q)) if q.size else 0.0


def check_step(label, tensors, exp, w, m, v, ratios):
    """every element of m, v, w and every r_T of a step inside its bar; prints the largest error / bar per quantity"""
    top = dict(m=0.0, v=0.0, w=0.0, r=0.0)
    for x in tensors:
        e = exp[x.name]
        got = dict(m=worst(m[x.sl], e.m, e.dm), v=worst(v[x.sl], e.v, e.dv), w=worst(w[x.sl], e.w, e.dw),
                   r=worst(np.asarray([ratios[x.name]]), np.asarray([e.r]), np.asarray([e.dr])))
        for k, q in got.items():
            assert q <= 1.0, (label, x.name, k, q)
            top[k] = max(top[k], q)
    print(f"[lamb] {label}: max error / bar  m {top['m']:.3f}  v {top['v']:.3f}  w {top['w']:.3f}  r {top['r']:.3f}")
    return top
