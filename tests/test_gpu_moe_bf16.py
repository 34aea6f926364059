"""bf16 AWQ-MoE: the expert-indirect forms of gemv_sharedx_bf16_kernel (16-row blocks, awq_aux_moe_gemv_blocks) and of
gemm_repacked_pipelined_bf16_kernel (128-row blocks, awq_aux_moe_gemm_blocks), and AWQMoEMethod.apply on them."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import awq_ref, c_oracle
from sglang_awq_amd import _lib, ops, synth
from sglang_awq_amd.awq import AWQConfig
from sglang_awq_amd.moe import AWQMoEMethod, select_experts
from tests.util import to_np, to_torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
vp = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _blocks(x, packed, row_map, block_expert, rows, y, K, N, g):
    lib = _lib.load()
    head = (vp(x), x.stride(0), 1, vp(packed), packed.stride(0), vp(row_map), vp(block_expert), block_expert.numel())
    tail = (None, vp(y), K, N, g, _lib.DTYPE_BF16, 0, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    return lib.awq_aux_moe_gemv_blocks(*head, *tail) if rows == 16 else lib.awq_aux_moe_gemm_blocks(*head, rows, *tail)


# K = 3200: 25 k-blocks (ragged last chunk of the GEMV, >= 3 chunks at every strip width); N = 1296: 81 column groups, neither whole
# strips nor whole 256-wide tiles.  Blocks: expert 2 with one real row | expert 0, full | unused | expert 1 with padding inside |
# expert 0 again, three rows.  Five pairs are never named: their rows must keep the sentinel.
@pytest.mark.parametrize("rows", [16, 128])
def test_one_hot_rows_through_row_map_reproduce_dequantize(rows):
    E, K, N, g = 3, 3200, 1296, 128
    w = [[to_torch(a, DEV) for a in synth.make_awq_weights(K, N, g, "bf16", "F", seed=40 + e)] for e in range(E)]
    W = torch.stack([ops.awq_dequantize(*w[e]) for e in range(E)])
    packed = torch.stack([ops.awq_repack(*w[e]) for e in range(E)])
    real = [np.array([3]), np.arange(rows), np.array([], dtype=int), np.arange(rows)[np.arange(rows) % 3 != 1], np.array([0, 1, rows - 1])]
    P = sum(len(r) for r in real) + 5
    pool = np.random.RandomState(rows).permutation(P)
    rm, block_expert, expert_of = np.full((5, rows), -1, dtype=np.int32), np.array([2, 0, -1, 1, 0], dtype=np.int32), np.full(P, -1)
    for b, r in enumerate(real):
        rm[b, r], pool = pool[:len(r)], pool[len(r):]
        expert_of[rm[b, r]] = block_expert[b]
    ks = (np.arange(P) * 131 + 17) % K
    edge = [0, 1, 2, 3, 4, 5, 6, 7, 127, 128, K - 129, K - 128] + list(range(K - 8, K))
    ks[np.nonzero(expert_of >= 0)[0][:len(edge)]] = edge                # first / last k-block, all eight nibble positions
    x = torch.zeros(P, K + 72, dtype=torch.bfloat16, device=DEV)[:, 8:8 + K]      # ldx > K
    x[torch.arange(P), torch.from_numpy(ks)] = 1.0
    y = torch.full((P, N), 7.0, dtype=torch.bfloat16, device=DEV)
    args = (x, packed, to_torch(rm.reshape(-1), DEV), to_torch(block_expert, DEV))
    assert _blocks(*args, rows, y, K, N, g) == 0
    named = torch.from_numpy(expert_of >= 0).to(DEV)
    want = W[torch.from_numpy(np.maximum(expert_of, 0)).to(DEV), torch.from_numpy(ks).to(DEV)]
    assert torch.equal(y[named], want[named])
    assert bool((y[~named] == 7.0).all()) and int((~named).sum()) == 5
    if rows == 128:
        assert _blocks(*args, 64, y, K, N, g) == _lib.ERR_BAD_VARIANT    # no 64-row bf16 tiles


E, K, I, TOP_K, G = 4, 3200, 640, 2, 128


@pytest.fixture(scope="module")
def experts():
    method, layer = AWQMoEMethod(AWQConfig(4, G, True)), torch.nn.Module()
    method.create_weights(layer, E, K, I, torch.bfloat16)
    w13 = [synth.make_awq_weights(K, 2 * I, G, "bf16", "A", seed=100 + e) for e in range(E)]
    w2 = [synth.make_awq_weights(I, K, G, "bf16", "A", seed=200 + e) for e in range(E)]
    for pre, ws in (("w13_", w13), ("w2_", w2)):
        for e in range(E):
            for name, a in zip(("qweight", "scales", "qzeros"), ws[e]):
                getattr(layer, pre + name).data[e].copy_(to_torch(a))
    layer.to(DEV)
    method.process_weights_after_loading(layer)
    return method, layer, w13, w2


def exact_sums(x, qw, s, qz):
    return c_oracle.gemm(x, qw, s, qz, want_exact=True)[1]


def compose(x, tw, ti, w13, w2, sums=exact_sums):
    """gate_up = bf16(sums), act = bf16(bf16(silu(gate)) * up), y = bf16(routed weight * sums), out = bf16(sum over the token's pairs);
    returns (out, sum |y|, sum w |act| @ |W2|) as float64."""
    r = lambda a: awq_ref.to_f64(awq_ref.from_f64(a, "bf16"), "bf16")
    want, scale, terms = (np.zeros((x.shape[0], K)) for _ in range(3))
    for e in range(E):
        absw2 = np.abs(awq_ref.to_f64(c_oracle.dequantize(*w2[e]), "bf16"))
        for k in range(TOP_K):
            t = np.nonzero(ti[:, k] == e)[0]
            if t.size:
                gu = r(sums(x[t], *w13[e]))
                act = r(r(gu[:, :I] / (1.0 + np.exp(-gu[:, :I]))) * gu[:, I:])
                ys = r(tw[t, k][:, None] * sums(awq_ref.from_f64(act, "bf16"), *w2[e]))
                want[t] += ys
                scale[t] += np.abs(ys)
                terms[t] += tw[t, k][:, None] * (np.abs(act) @ absw2)
    return r(want), scale, terms


def tolerance(scale, terms):
    return 2.5 * 2.0 ** (np.floor(np.log2(np.maximum(scale, 2.0 ** -14))) - 7) + 2e-3 * (1.0 + scale) + 2.0 ** -10 * terms


def routing(T):
    logits = synth.make_activations(T, E, "f16", "A", seed=T + 50).astype(np.float32)
    if T == 24:
        logits[:, 1] += 20.0                                            # expert 1 takes every token: two 16-row blocks of it
    if T == 150:
        logits[:, 0] += 20.0                                            # expert 0 takes every token (two 128-row tiles), expert 3 none
        logits[:, 3] -= 20.0
    tw, ti = select_experts(torch.from_numpy(logits), TOP_K)
    if T == 150:
        ti[-4:] = -1                                                    # padded tokens of a graph batch: rows of exact zeros
    return tw, ti


@pytest.mark.parametrize("T", [1, 5, 24, 150])
def test_awq_moe_method_bf16_vs_oracle(experts, T):
    """2, 10, 48 pairs on 16-row blocks, 150 tokens on 128-row tiles.  Tolerance: test_awq_moe_method_vs_oracle's with fp16's 10 mantissa
    bits replaced by bf16's 7 in each ulp term: 2.5 * 2^(floor(log2 scale) - 7) + 2e-3 (1 + scale) + 2^-10 terms.  The same composition
    with numpy float32 matmuls on the dequantised weights in place of the exact sums stays inside it on the CPU (worst err / tolerance
    0.00 / 0.08 / 0.25 / 0.30 at T = 1 / 5 / 24 / 150), so the act-ulp term 2^-10 is not widened."""
    method, layer, w13, w2 = experts
    x = synth.make_activations(T, K, "bf16", "A", seed=T, x_std=0.5)
    tw, ti = (a.to(DEV) for a in routing(T))
    xt = to_torch(x, DEV)
    out_t = method.apply(layer, xt, tw, ti)
    assert out_t.dtype == torch.bfloat16 and out_t.shape == (T, K)
    out = awq_ref.to_f64(to_np(out_t), "bf16")
    want, scale, terms = compose(x, tw.cpu().numpy().astype(np.float64), ti.cpu().numpy(), w13, w2)
    err, tol = np.abs(out - want), tolerance(scale, terms)
    print(f"T={T}: worst err / tolerance {(err / tol).max():.3f}, {float((out != want).mean()):.4f} of elements differ")
    assert np.all(err <= tol), f"T={T}: {int((err > tol).sum())} of {err.size} outside, worst err / tolerance {(err / tol).max():.3f}"
    if T == 150:
        assert not out_t[-4:].any()
    if T in (5, 150):                                                   # one T per route: capture, replay twice, same bits
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        gph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gph, stream=side):
            captured = method.apply(layer, xt, tw, ti)
        gph.replay()
        gph.replay()
        torch.cuda.synchronize()
        assert torch.equal(captured, out_t)
