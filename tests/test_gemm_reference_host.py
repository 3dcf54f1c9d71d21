"""tests/gemm_reference.py checked on the host: a numpy model of the GEMM kernels' arithmetic -- exact fp32 products of bf16 values,
summed in fp32 in several orders, cut into k-slabs and reduced, the epilogue in fp32, a round-to-nearest-even bf16 store -- has to stay
inside `bars` at every shape class tests/test_gemm_kernels_gpu.py uses (M and N scaled down, K and the split counts as there), has to
reproduce the fp64 reference BIT FOR BIT on `exact_operands` in every order, and two broken models (one product dropped; truncating bf16
stores) have to be caught -- the bars and the exact check are not vacuous.  Prints the largest error / bar per form (`-s`).  No GPU."""
import numpy as np
import pytest
import torch

import gemm_reference as R

M_, N_ = 9, 16
ORDERS = ("sequential", "chunks16", "pairwise")
# K of every shape class of the GPU file -> the split counts modelled with it (1 = no cut)
K_BF16 = [8, 64, 72, 128, 192, 200, 320, 1024]
K_TN = {1: (1,), 40: (1,), 300: (1,), 333: (1,), 5000: (5, 16), 70000: (17, 64), 5120: (10,), 5160: (10,), 7168: (14,)}
K_NT_F32 = {8: (1,), 72: (1,), 200: (1,), 1024: (1,), 5120: (1, 10)}       # (the bias form is never cut: splits = 1 only)


@pytest.fixture(scope="module")
def pools():
    g = torch.Generator().manual_seed(20240)
    return R.exact_pool(g, M_, N_, 70000), R.normal_pool(g, M_, N_, 70000)


def fsum(P, order):
    """fp32 sum over the last axis in the given order"""
    P = np.asarray(P, dtype=np.float32)
    if P.shape[-1] == 0:
        return np.zeros(P.shape[:-1], np.float32)
    if order == "sequential":
        return np.cumsum(P, axis=-1, dtype=np.float32)[..., -1]        # (cumsum adds left to right in its dtype)
    if order == "chunks16":
        pad = (-P.shape[-1]) % 16
        Q = np.concatenate((P, np.zeros(P.shape[:-1] + (pad,), np.float32)), -1).reshape(P.shape[:-1] + (-1, 16))
        return fsum(fsum(Q, "sequential"), "sequential")
    n = 1 << (P.shape[-1] - 1).bit_length()
    Q = np.concatenate((P, np.zeros(P.shape[:-1] + (n - P.shape[-1],), np.float32)), -1)
    while Q.shape[-1] > 1:
        h = Q.shape[-1] // 2
        Q = Q[..., :h] + Q[..., h:]
    return Q[..., 0]


def ksum(P, order, splits):
    """the k sum as the kernels cut it: k-tiles of 64 dealt to `splits` slabs, each summed on its own, the partials added in a fixed order
    (up to 16: one after the other; more: eight interleaved chains, then folded, as splitk_reduce_deep_kernel does)"""
    if splits == 1:
        return fsum(P, order)
    K = P.shape[-1]
    nk = (K + 63) // 64
    per = (nk + splits - 1) // splits
    parts = [fsum(P[..., s * per * 64:(s + 1) * per * 64], order) for s in range((nk + per - 1) // per)]
    if len(parts) <= 16:
        return fsum(np.stack(parts, -1), "sequential")
    lanes = [fsum(np.stack(parts[l::8], -1), "sequential") for l in range(8)]
    return fsum(np.stack(lanes, -1), "sequential")


def gelu_model(x):
    """gelu_pair of csrc/common.h in fp32: Phi(x) ~ sigmoid(x (c0 + c1 u + c2 u^2)), u = min(x^2, U_MAX)"""
    f = np.float32
    C0, C1, C2 = f(1.5949398799788077), f(0.07403000634661838), f(-0.0007007124749191571)
    x = x.astype(np.float32)
    u = np.minimum(x * x, C1 / (f(2.0) * -C2))
    with np.errstate(over="ignore"):
        s = (f(1.0) / (np.exp(-(x * ((u * C2 + C1) * u + C0)), dtype=np.float32) + f(1.0))).astype(np.float32)
    act = x * s
    q = (u * (f(5.0) * C2) + f(3.0) * C1) * u + C0
    return act, (act * (f(1.0) - s)) * q + s


def model(form, ops, order="sequential", splits=1, store=R.np_bf16_rne, drop=None, stored_colsum=False, round_pre=False):
    """the outputs of `form` as a kernel of this family computes them, as fp64 torch tensors.  drop = (m, n, k): that product is left out."""
    f = np.float32
    A, B = ops["A"].numpy().astype(f), ops["B"].numpy().astype(f)
    P = A[:, None, :] * B.T[None, :, :]                  # [M, N, K]: products of bf16 values are exact in fp32
    if drop is not None:
        P[drop] = 0.0
    v = ksum(P, order, splits)
    epi = form.epi
    if epi in R.HAS_BIAS:
        v = v + ops["bias"].numpy().astype(f)
    if epi == R.EPI_BIAS and ops["qcols"]:
        v[:, :ops["qcols"]] *= f(ops["qscale"])
    out = {}
    if epi in R.GELU:
        v, der = gelu_model(R.np_bf16_rne(v) if round_pre else v)
        if epi == R.EPI_BIAS_GELU:
            out["C2"] = store(der)
    if epi in (R.EPI_ADD, R.EPI_BIAS_ADD):
        v = v + ops["aux"].numpy().astype(f)
    if epi in (R.EPI_DGELU, R.EPI_DGELU_COLSUM):
        v = v * ops["aux"].numpy().astype(f)
    if epi == R.EPI_DGELU_COLSUM:
        terms = store(v) if stored_colsum else v
        out["C2"] = fsum(terms.T, order) + ops["prior2"].numpy().astype(f)
    if form.aks and form.f32 and form.c2:
        out["C2"] = ksum(A, order, splits) + ops["prior2"].numpy().astype(f)
    if form.acc:
        v = v + ops["prior"].numpy().astype(f)
    out["C"] = v if form.f32 else store(v)
    return {k: torch.from_numpy(np.ascontiguousarray(x)).to(R.F64) for k, x in out.items()}


def cases():
    for form in R.NT_BF16 + R.NN_BF16:
        for K in K_BF16:
            yield form, K, 1
    for form in R.TN_F32:
        for K, cuts in K_TN.items():
            for s in cuts:
                yield form, K, s
    for form in R.NT_F32:
        for K, cuts in K_NT_F32.items():
            for s in cuts:
                if s == 1 or form.epi == R.EPI_NONE:
                    yield form, K, s


def test_reference_against_a_plain_loop():
    g = torch.Generator().manual_seed(3)
    A, B = torch.randn((3, 5), generator=g).double(), torch.randn((5, 4), generator=g).double()
    bias, aux, prior = torch.randn(4, generator=g).double(), torch.randn((3, 4), generator=g).double(), torch.randn((3, 4), generator=g).double()
    acc = torch.tensor([[sum(float(A[m, k]) * float(B[k, n]) for k in range(5)) for n in range(4)] for m in range(3)], dtype=R.F64)
    close = lambda a, b: float((a - b).abs().max()) < 1e-13
    assert close(R.reference(R.FORMS["nt"], A, B)["C"], acc)
    assert close(R.reference(R.FORMS["nt+bias_add"], A, B, bias, aux)["C"], acc + bias + aux)
    r = R.reference(R.FORMS["nt+bias,qcols"], A, B, bias, qcols=2, qscale=0.25)["C"]
    assert close(r[:, :2], (acc + bias)[:, :2] * 0.25) and close(r[:, 2:], (acc + bias)[:, 2:])
    r = R.reference(R.FORMS["nt*dgelu+colsum"], A, B, aux=aux, prior2=bias)
    assert close(r["C"], acc * aux) and close(r["C2"], (acc * aux).sum(0) + bias)
    r = R.reference(R.FORMS["tn_f32+rowsum+acc"], A, B, prior=prior, prior2=bias[:3])
    assert close(r["C"], acc + prior) and close(r["C2"], A.sum(1) + bias[:3])
    x = R.bf16_round(acc + bias)
    assert bool((x.to(torch.bfloat16).double() == x).all()) and float(((acc + bias) - x).abs().max()) > 0
    r = R.reference(R.FORMS["nt+bias_gelu"], A, B, bias)
    xg = x.clone().requires_grad_(True)
    y = torch.nn.functional.gelu(xg)
    y.sum().backward()
    assert close(r["C"], y.detach()) and close(r["C2"], xg.grad)
    assert close(R.reference(R.FORMS["nt+bias_gelu_act"], A, B, bias)["C"], y.detach())


def test_bf16_round_is_one_rounding_to_nearest_even():
    x = torch.tensor([1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 1.0 + 2.0 ** -8 + 2.0 ** -40, -(1.0 + 2.0 ** -8), 0.0, 3.0e-5, 255.5, 1.0 + 2.0 ** -8 - 2.0 ** -30],
                     dtype=R.F64)
    want = torch.tensor([1.0, 1.0 + 2.0 ** -6, 1.0 + 2.0 ** -7, -1.0, 0.0, float(torch.tensor(3.0e-5).to(torch.bfloat16)), 256.0, 1.0], dtype=R.F64)
    assert torch.equal(R.bf16_round(x), want)
    y = torch.randn(4096, dtype=torch.float32)
    assert torch.equal(R.bf16_round(y.double()), y.to(torch.bfloat16).double())
    assert np.array_equal(R.np_bf16_rne(y.numpy()), y.to(torch.bfloat16).float().numpy())


def test_model_stays_inside_the_bars_and_is_exact_on_exact_operands(pools):
    epool, npool = pools
    worst = {}
    for form, K, splits in cases():
        qcols = 8 if form.q else 0
        ex = R.exact_operands(epool, form, M_, N_, K, qcols=qcols)
        no = R.normal_operands(npool, form, M_, N_, K, qcols=qcols)
        for stored in ((False, True) if form.epi == R.EPI_DGELU_COLSUM else (False,)):
            ebar = R.bars_of(form, ex, splits, exact=True, stored_colsum=stored)
            nbar = R.bars_of(form, no, splits, stored_colsum=stored)
            for order in ORDERS:
                got = model(form, ex, order, splits, stored_colsum=stored)
                for key, want in ex["ref"].items():
                    if form.epi in R.GELU:
                        assert R.first_bad(got[key], want, ebar[key]) is None, (form.name, K, splits, order, key, R.first_bad(got[key], want, ebar[key]))
                        worst[(form.name + " exact", key)] = max(worst.get((form.name + " exact", key), 0.0), R.worst_ratio(got[key], want, ebar[key]))
                    else:
                        assert float(ebar[key].max()) == 0.0
                        assert torch.equal(got[key], want), (form.name, K, splits, order, key, R.first_bad(got[key], want, ebar[key]))
                got = model(form, no, order, splits, stored_colsum=stored)
                for key, want in no["ref"].items():
                    assert R.first_bad(got[key], want, nbar[key]) is None, (form.name, K, splits, order, key, R.first_bad(got[key], want, nbar[key]))
                    worst[(form.name, key)] = max(worst.get((form.name, key), 0.0), R.worst_ratio(got[key], want, nbar[key]))
    for (name, key), r in sorted(worst.items()):
        print("model  %-28s %-2s  worst error / bar %.3f" % (name, key, r))
    assert worst and max(worst.values()) < 1.0


def test_exact_check_catches_one_dropped_product(pools):
    epool, _ = pools
    for name, K, splits in (("nt", 1024, 1), ("nn+add", 192, 1), ("nt+bias,qcols", 72, 1), ("tn_f32", 5000, 5), ("nt_f32+bias", 1024, 1),
                            ("nt*dgelu+colsum", 200, 1)):
        form = R.FORMS[name]
        ex = R.exact_operands(epool, form, M_, N_, K, qcols=8 if form.q else 0)
        prod = ex["A"][:, None, :] * ex["B"].t()[None, :, :]
        if ex["aux"] is not None and form.epi in (R.EPI_DGELU, R.EPI_DGELU_COLSUM):
            prod = prod * ex["aux"][:, :, None]
        m, n, k = (int(i) for i in torch.nonzero(prod)[-1])
        got = model(form, ex, "pairwise", splits, drop=(m, n, k))
        bad = ~(got["C"] == ex["ref"]["C"])
        assert int(bad.sum()) == 1 and bool(bad[m, n]), (name, int(bad.sum()))
        assert "(m %d, n %d)" % (m, n) in R.first_bad(got["C"], ex["ref"]["C"], torch.zeros_like(got["C"]))
        if form.epi == R.EPI_DGELU_COLSUM:
            assert not torch.equal(got["C2"], ex["ref"]["C2"])
        # ... and on ordinary operands the dropped product is far outside the bar of its element, where the norm test saw 1 % of the tensor
        if name == "nt":
            no = R.normal_operands(pools[1], form, M_, N_, K)
            prod = (no["A"][:, None, :] * no["B"].t()[None, :, :]).abs()
            m, n, k = (int(i) for i in torch.nonzero(prod == prod.max())[0])
            got = model(form, no, "pairwise", 1, drop=(m, n, k))
            assert R.first_bad(got["C"], no["ref"]["C"], R.bars_of(form, no)["C"]) is not None


def test_bars_catch_truncating_bf16_stores(pools):
    """(the GELU forms on their exact operands, where the pre-activation is a bf16 number: on ordinary ones the allowance for the
    argument's rounding is as large as a truncated store's error)"""
    epool, npool = pools
    for form in R.NT_BF16 + R.NN_BF16:
        if form.epi in R.GELU:
            no = R.exact_operands(epool, form, M_, N_, 192)
            bar = R.bars_of(form, no, exact=True)
        else:
            no = R.normal_operands(npool, form, M_, N_, 192, qcols=8 if form.q else 0)
            bar = R.bars_of(form, no)
        got = model(form, no, "chunks16", store=R.np_bf16_trunc)
        assert R.first_bad(got["C"], no["ref"]["C"], bar["C"]) is not None, form.name
        if form.epi == R.EPI_BIAS_GELU:
            assert R.first_bad(got["C2"], no["ref"]["C2"], bar["C2"]) is not None


def test_gelu_bar_needs_the_preactivation_rounding_term(pools):
    """The header defines the GELU forms at x = bf16(acc + bias); the epilogues evaluate at the fp32 sum.  A model that rounds x first stays
    inside the bar WITHOUT the 2^-8 |x| term; the model of what the kernels do (no rounding) does not -- so the term is what that difference
    costs and nothing else -- and stays inside the bar with it."""
    # the GEMM of test_gemm_gelu_epilogue_accuracy: A a one-hot column, B zeros, so x = the fp32 bias itself -- a dense sweep of fp32
    # pre-activations over [-8, 8], most of which are no bf16 numbers
    form = R.FORMS["nt+bias_gelu"]
    n = 1 << 18
    ops = {"A": torch.ones(1, 8), "B": torch.zeros(8, n), "bias": torch.linspace(-8, 8, n), "aux": None, "prior": None, "prior2": None, "qcols": 0,
           "qscale": 1.0}
    ref, bar = R.ref_of(form, ops), R.bars_of(form, ops)
    pre = R.d(ops["bias"]).abs()[None, :]
    without = {"C": bar["C"] - R.GELU_SLOPE * R.BF16_STORE * pre, "C2": bar["C2"] - R.GELU_CURV * R.BF16_STORE * pre}
    rounded, plain = model(form, ops, round_pre=True), model(form, ops)
    for key in ("C", "C2"):
        assert R.first_bad(rounded[key], ref[key], without[key]) is None, (key, R.first_bad(rounded[key], ref[key], without[key]))
        assert R.first_bad(plain[key], ref[key], bar[key]) is None, (key, R.first_bad(plain[key], ref[key], bar[key]))
        print("gelu sweep %-2s  rounded x: %.3f of the bar without the term;  fp32 x: %.3f of it, %.3f of the bar with the term" % (
            key, R.worst_ratio(rounded[key], ref[key], without[key]), R.worst_ratio(plain[key], ref[key], without[key]),
            R.worst_ratio(plain[key], ref[key], bar[key])))
    assert any(R.first_bad(plain[key], ref[key], without[key]) is not None for key in ("C", "C2"))


def test_exact_operands_refuses_sums_the_type_cannot_hold(pools):
    """the builder's own precondition check is live: operands whose sums leave bf16's 8 bits are refused"""
    epool = dict(pools[0])
    epool["A"] = torch.ones_like(epool["A"])
    epool["B"] = torch.ones_like(epool["B"])
    with pytest.raises(AssertionError):
        R.exact_operands(epool, R.FORMS["nt"], M_, N_, 1001)
    R.exact_operands(epool, R.FORMS["nt_f32"], M_, N_, 1001)       # fp32 holds 1001
    # straight from a generator, no pool: the same precondition, the same reference
    ex = R.exact_operands(torch.Generator().manual_seed(1), R.FORMS["nt+bias_add"], 5, 8, 72)
    assert ex["A"].shape == (5, 72) and torch.equal(ex["ref"]["C"], R.d(ex["A"]) @ R.d(ex["B"]) + R.d(ex["bias"]) + R.d(ex["aux"]))
