"""ia_gemm_dgrad_rows: the data gradient dX = dY W (+ epilogue) that computes only the 32-row blocks holding a live row and writes the
others as zeros, against the unfiltered call (ia_gemm_bf16, data-gradient form) on the same inputs, element for element.

Shapes: M = 20 x 255 = 5100 rows (159 whole blocks and one of 12 rows), N = 2048: 20 x 8 = 160 tiles of 256 x 256, the smallest plan the
256-wide kernel takes (ia_gemm_dgrad_rows_filters is asserted); K = 64 (one k-tile), 192 (three) and 1024.  Every epilogue the filter
serves (NONE, ADD, DGELU_COLSUM) with W read k-strided and through its transposed copy.  C is filled with NaN before every call, so a
row nobody wrote shows.  N = 4096 (320 tiles on 256 workgroups, plain epilogue, transposed W) reaches the look-ahead kernel's remapped form.

Column sums (DGELU_COLSUM): the filtered and the unfiltered call add the same fp32 terms in two groupings, so each is compared with the
fp64 column sum of the bf16 output (on the CPU) and the filtered error may be at most twice the unfiltered one.  Measured on MI355X,
largest absolute error over all masks and K (at K = 1024, every row live, sums of 5100 terms of magnitude ~13): filtered 5.492e+00,
unfiltered 5.492e+00, for W k-strided and transposed alike; the smallest non-zero pair, one live row at K = 64: 2.981e-02 both.  Both are
dominated by the bf16 rounding of the output the reference sums (the kernels add the fp32 values in front of that rounding); the two
groupings differ in the fourth digit at most (five live blocks, K = 1024: 9.342e-01 against 9.343e-01)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

BLK = 32
M, N, L = 5100, 2048, 255
KS = (64, 192, 1024)
EPI_NONE, EPI_ADD, EPI_DGELU_COLSUM = 0, 3, 6


def masks():
    """name -> row_live (numpy uint8 [M])"""
    nb = (M + BLK - 1) // BLK
    out = {}
    rs = np.random.RandomState(77)
    live = np.zeros(M, np.uint8)                       # right-padded sequences, lengths as the benchmark's synthetic data draws them
    for b in range(M // L):
        live[b * L: b * L + 3 + rs.randint(8, 49) + rs.randint(16, 204)] = 1
    live[(M // L - 1) * L + 60: M] = 0                 # the last sequence short: the partial last block is dead
    out["padded"] = live
    out["all_live"] = np.ones(M, np.uint8)             # ... and here it is live
    out["all_dead"] = np.zeros(M, np.uint8)
    few = np.zeros(M, np.uint8); few[100:250] = 1      # blocks 3 .. 7: fewer than eight, one tile
    out["five_blocks"] = few
    odd = np.zeros(M, np.uint8); odd[: 13 * BLK] = 1; odd[40 * BLK: 46 * BLK] = 1; odd[M - 5:] = 1      # 13 + 6 + 1 = 20 blocks: 2.5 tiles, the partial block the last
    out["twenty_blocks"] = odd
    one = np.zeros(M, np.uint8); one[1000] = 1         # a single live row inside an otherwise dead block
    out["one_row"] = one
    mix = live.copy(); mix[3000] = 1; mix[3000 - 2 * BLK] = 0
    out["padded_plus_one_row"] = mix
    for name, m in out.items():
        assert len(m) == M, name
    assert not out["padded"][(nb - 1) * BLK:].any()
    return out


@pytest.fixture(scope="module")
def operands(gpu):
    g = torch.Generator(device="cpu").manual_seed(4321)
    kmax = max(KS)
    return {"dy": torch.randn((M, kmax), generator=g).to(gpu).to(torch.bfloat16),
            "w": (torch.randn((kmax, N), generator=g) * 0.4).to(gpu).to(torch.bfloat16),
            "aux": torch.randn((M, N), generator=g).to(gpu).to(torch.bfloat16)}


def test_row_blocks_kernel_matches_host(gpu):
    from item_alignment_amd import _lib, ops
    lib = _lib.load()
    rs = np.random.RandomState(5)
    patterns = list(masks().values()) + [(rs.rand(130560) < 0.01).astype(np.uint8), np.ones(33, np.uint8), np.zeros(1, np.uint8)]
    for live in patterns:
        for off in (0, 3):                 # an unaligned row_live pointer too
            buf = torch.zeros(len(live) + off, dtype=torch.uint8)
            buf[off:] = torch.from_numpy(live)
            got = ops.row_blocks(buf.to(gpu)[off:]).cpu().numpy()
            want = np.zeros_like(got)
            assert lib.ia_row_blocks_host(live.ctypes.data, len(live), want.ctypes.data) == 0
            nbr = (want[2] + 7) // 8 * 8
            assert np.array_equal(got[:8], want[:8])
            assert np.array_equal(got[8: 8 + want[0]], want[8: 8 + want[0]])
            assert np.array_equal(got[8 + nbr: 8 + nbr + want[1]], want[8 + nbr: 8 + nbr + want[1]])


@pytest.mark.parametrize("w_kstrided", [True, False], ids=["w_kstrided", "w_transposed"])
@pytest.mark.parametrize("epilogue", [EPI_NONE, EPI_ADD, EPI_DGELU_COLSUM], ids=["none", "add", "dgelu_colsum"])
def test_dgrad_rows_equals_unfiltered(gpu, operands, epilogue, w_kstrided):
    from item_alignment_amd import _lib, ops
    lib = _lib.load()
    nan = lambda: torch.full((M, N), float("nan"), device=gpu, dtype=torch.bfloat16)
    worst_f = worst_d = 0.0
    for K in KS:
        assert lib.ia_gemm_dgrad_rows_filters(M, N, K) == 1
        w = operands["w"][:K].contiguous()
        b = w if w_kstrided else w.t().contiguous()
        for name, live_np in masks().items():
            live = torch.from_numpy(live_np).to(gpu)
            keep = live[:, None].to(torch.bfloat16)
            dy = (operands["dy"][:, :K] * keep).contiguous()              # the contract: dead rows of dY are zero ...
            aux = None
            if epilogue == EPI_ADD:
                aux = (operands["aux"] * keep).contiguous()                # ... and of aux, where it is added
            elif epilogue == EPI_DGELU_COLSUM:
                aux = operands["aux"]                                      # (a saved gelu' is not zero at a padded position)
            cs_d = torch.zeros(N, device=gpu) if epilogue == EPI_DGELU_COLSUM else None
            cs_f = torch.zeros(N, device=gpu) if epilogue == EPI_DGELU_COLSUM else None
            dense = ops.gemm(dy, b, b_kstrided=w_kstrided, epilogue=epilogue, aux=aux, out=nan(), colsum_out=cs_d)
            got = ops.gemm_dgrad_rows(dy, b, live, w_kstrided=w_kstrided, epilogue=epilogue, aux=aux, out=nan(), colsum_out=cs_f)
            tag = (K, name)
            assert not torch.isnan(got).any(), tag                         # every row was written
            assert torch.equal(got, dense), tag                            # all rows: live ones as computed, dead ones zero (+-0 compare equal)
            dead_rows = torch.from_numpy(np.repeat([not live_np[t * BLK: (t + 1) * BLK].any() for t in range((M + BLK - 1) // BLK)], BLK)[:M]).to(gpu)
            assert got[dead_rows].abs().max().item() == 0.0 if dead_rows.any() else True, tag
            if name == "all_dead":
                assert got.abs().max().item() == 0.0
            # NULL = the unfiltered call
            if name == "padded":
                assert torch.equal(ops.gemm_dgrad_rows(dy, b, None, w_kstrided=w_kstrided, epilogue=epilogue, aux=aux, out=nan(),
                                                       colsum_out=torch.zeros(N, device=gpu) if cs_d is not None else None), dense), tag
            # large values in the rows of blocks that are dead as a whole (the rows of partly live blocks stay zero: the contract needs
            # them zero): a kernel that read those blocks could not return the clean result
            if dead_rows.any():
                sign = torch.where(torch.arange(K, device=gpu) % 2 == 0, 1e4, -1e4).to(torch.bfloat16)
                dyp = torch.where(dead_rows[:, None], sign[None, :], dy).contiguous()
                cs_p = torch.zeros(N, device=gpu) if cs_d is not None else None
                gotp = ops.gemm_dgrad_rows(dyp, b, live, w_kstrided=w_kstrided, epilogue=epilogue, aux=aux, out=nan(), colsum_out=cs_p)
                assert torch.equal(gotp, got), tag
                if cs_p is not None:
                    assert torch.equal(cs_p, cs_f), tag
            if epilogue == EPI_DGELU_COLSUM:
                ref = got.cpu().double().sum(0)
                e_f = (cs_f.cpu().double() - ref).abs().max().item()
                e_d = (cs_d.cpu().double() - ref).abs().max().item()
                print(f"K {K} {name}: column sums vs fp64: filtered {e_f:.3e}, unfiltered {e_d:.3e}")
                worst_f, worst_d = max(worst_f, e_f), max(worst_d, e_d)
                assert e_f <= 2.0 * e_d, (tag, e_f, e_d)
    if epilogue == EPI_DGELU_COLSUM:
        print(f"largest column-sum error: filtered {worst_f:.3e}, unfiltered {worst_d:.3e}")


def test_dgrad_rows_lookahead_kernel(gpu, operands):
    """More tiles than workgroups (N = 4096: 20 x 16 = 320 tiles on 256) with both operands k-contiguous and the plain epilogue is the
    look-ahead kernel's shape: its remapped form takes the current tile's and the NEXT tile's row bases from the list.  K = 128 is the
    shortest K it serves (two k-tiles: every trip looks into the next tile), 320 has a K tail."""
    from item_alignment_amd import _lib, ops
    lib = _lib.load()
    n = 4096
    g = torch.Generator(device="cpu").manual_seed(99)
    wt_all = (torch.randn((n, 320), generator=g) * 0.4).to(gpu).to(torch.bfloat16)
    nan = lambda: torch.full((M, n), float("nan"), device=gpu, dtype=torch.bfloat16)
    for K in (128, 320):
        assert lib.ia_gemm_dgrad_rows_filters(M, n, K) == 1
        wt = wt_all[:, :K].contiguous()
        for name, live_np in masks().items():
            live = torch.from_numpy(live_np).to(gpu)
            dy = (operands["dy"][:, :K] * live[:, None].to(torch.bfloat16)).contiguous()
            dense = ops.gemm(dy, wt, out=nan())
            got = ops.gemm_dgrad_rows(dy, wt, live, w_kstrided=False, out=nan())
            assert not torch.isnan(got).any(), (K, name)
            assert torch.equal(got, dense), (K, name)
            dead_rows = torch.from_numpy(np.repeat([not live_np[t * BLK: (t + 1) * BLK].any() for t in range((M + BLK - 1) // BLK)], BLK)[:M]).to(gpu)
            if dead_rows.any():                    # blocks that are dead as a whole are not read
                dyp = torch.where(dead_rows[:, None], torch.tensor(1e4, device=gpu, dtype=torch.bfloat16), dy).contiguous()
                assert torch.equal(ops.gemm_dgrad_rows(dyp, wt, live, w_kstrided=False, out=nan()), got), (K, name)
