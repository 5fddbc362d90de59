"""CPU side of the attention-variant tests: the float64 reference against PyTorch's own attention, the input builders against what
they promise, and the shape tables against the library's dispatch.  The last part is what makes "every variant" true: the queries
sbgm_*_variant are the functions the launchers themselves call, and they need no device."""
import ctypes as C
import math

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import attention_ref as R
import attention_variant_shapes as T
from sbgm_danra_amd import _native as N


def fwd_query(B, S, C_, heads):
    info = (C.c_int * 4)()
    vid = N.lib().sbgm_mha_core_fwd_variant(B, S, C_, heads, info)
    return vid, tuple(info)


def bwd_query(B, S, C_, heads):
    info = (C.c_int * 4)()
    vid = N.lib().sbgm_mha_core_bwd_variant(B, S, C_, heads, info)
    return vid, tuple(info)


def tok_query(M, C_):
    info = (C.c_int * 2)()
    vid = N.lib().sbgm_attn_tokens_variant(M, C_, info)
    return vid, tuple(info)


# ---- the reference ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,S,C_,heads", [(2, 17, 24, 2), (1, 40, 32, 4)])
def test_reference_equals_torch_attention(B, S, C_, heads):
    qkv = R.plain(B, S, C_, heads).double()
    q, k, v = R.split_heads(qkv, heads)
    want = F.scaled_dot_product_attention(q, k, v).transpose(1, 2).reshape(B, S, C_)
    assert torch.allclose(R.mha_core(qkv, heads), want, rtol=1e-13, atol=1e-14)
    dout = torch.randn(B, S, C_, generator=R.gen(1), dtype=torch.float64)
    x = qkv.clone().requires_grad_(True)
    F.scaled_dot_product_attention(*R.split_heads(x, heads)).transpose(1, 2).reshape(B, S, C_).backward(dout)
    assert torch.allclose(R.mha_core_grad(qkv, dout, heads), x.grad, rtol=1e-12, atol=1e-13)


def test_reference_equals_multihead_attention_pieces():
    """in_proj -> core -> out_proj of nn.MultiheadAttention, and the token-block expressions around it, in float64"""
    B, S, C_, heads = 2, 9, 64, 4
    g = R.gen(2)
    mha = nn.MultiheadAttention(C_, heads, batch_first=True).double()
    ln1, ln2 = nn.LayerNorm(C_).double(), nn.LayerNorm(C_).double()
    ff = nn.Sequential(nn.Linear(C_, C_), nn.GELU(), nn.Linear(C_, C_)).double()
    with torch.no_grad():
        for p in [*mha.parameters(), *ln1.parameters(), *ln2.parameters(), *ff.parameters()]:
            p.copy_(torch.randn(p.shape, generator=g, dtype=torch.float64) * 0.2 + (1.0 if p.ndim == 1 else 0.0))
        x = torch.randn(B, S, C_, generator=g, dtype=torch.float64)
        xn = ln1(x)
        a, _ = mha(xn, xn, xn)
        h = a + x
        want = ff(ln2(h)) + h
        qkv = R.attn_in(x, ln1.weight, ln1.bias, mha.in_proj_weight, mha.in_proj_bias)
        att = R.mha_core(qkv, heads)
        got = R.attn_tail(att, x, mha.out_proj.weight, mha.out_proj.bias, ln2.weight, ln2.bias, ff[0].weight, ff[0].bias,
                          ff[2].weight, ff[2].bias)
    assert torch.allclose(got, want, rtol=1e-12, atol=1e-13)


def test_row_error_finds_one_bad_row():
    want = torch.randn(2, 50, 3 * 8, generator=R.gen(3), dtype=torch.float64)
    got = want.clone()
    got[1, 37, 8 + 5] += 1e-3                       # head 1, row 37
    err = R.row_error(got, want, heads=3)
    val, where = R.worst_row(err)
    assert where == (1, 1, 37) and val == pytest.approx(1e-3 / float(want[1, 37, 8:16].abs().max()))
    assert int((err > 0).sum()) == 1
    got[0, 3, 0] = float("nan")
    assert R.worst_row(R.row_error(got, want, heads=3)) == (float("inf"), (0, 0, 3))
    head = R.head_error(got, want, heads=3)
    assert torch.isinf(head[0, 0, 3]) and int((head > 0).sum()) == 2
    assert float(head[1, 1, 37]) == pytest.approx(1e-3 / float(want[1, :, 8:16].abs().max()))
    assert R.tolerance(torch.tensor([1e-9])) == R.FLOOR and R.tolerance(torch.tensor([1e-6, 3e-6])) == pytest.approx(1.2e-5)


# ---- the builders ----------------------------------------------------------------------------------------------------------------
FWD_SHAPES = sorted({(B, S, C_, heads) for B, S, C_, heads, e in T.FWD if e != T.REFUSED})
SMALL_FWD = [s for s in FWD_SHAPES if s[0] * s[3] * s[1] * s[1] <= 1 << 21]


@pytest.mark.parametrize("B,S,C_,heads", FWD_SHAPES)
def test_gather_builder_concentrates_every_row(B, S, C_, heads):
    """every shape of the forward table: row i keeps more than 1 - 1e-6 of its float64 mass on key pi(i), pi is a permutation"""
    qkv, pi, v = R.gather(B, S, C_, heads)
    assert qkv.dtype == torch.float32 and torch.isfinite(qkv).all()
    assert torch.equal(torch.sort(pi, -1).values, torch.arange(S).expand(B, heads, S))
    assert (pi[:, :, 0] == S - 1).all() and (pi[:, :, S - 1] == 0).all()
    top = torch.gather(R.probabilities(qkv, heads), 3, pi[..., None])
    assert float(top.min()) > 1 - R.GATHER_MASS
    exp = R.gather_expected(pi, v)
    assert torch.equal(exp.double().float(), exp) and float((R.mha_core(qkv, heads) - exp).abs().max()) < 2e-3
    bound = R.gather_bound(qkv, heads, exp)
    assert float((bound / exp.abs()).max()) < 1e-4             # the bound itself stays a localised check: far below the gap between two keys


@pytest.mark.parametrize("B,S,C_,heads", SMALL_FWD[::4])
def test_offset_and_spike_builders(B, S, C_, heads):
    d = C_ // heads
    qkv = R.offset(B, S, C_, heads)
    q, k, _ = R.split_heads(qkv.double(), heads)
    logits = q @ k.transpose(-1, -2) / math.sqrt(d)
    assert float(logits.min()) > 89.0, "every logit overflows exp() in fp32 unless the row maximum is subtracted"
    assert abs(float(qkv[..., :C_].mean()) - 3.0) < 0.2 and abs(float(qkv[..., 2 * C_:].mean()) - 3.0) < 0.2
    assert torch.isfinite(R.mha_core(qkv, heads, torch.float32)).all()
    for pos in R.spike_positions(S):
        sp, base = R.late_spike(B, S, C_, heads, pos), R.plain(B, S, C_, heads, 2)
        assert torch.equal(sp[:, pos, C_:2 * C_], base[:, pos, C_:2 * C_] * R.SPIKE)
        sp[:, pos, C_:2 * C_] = base[:, pos, C_:2 * C_]
        assert torch.equal(sp, base)
        # some query of every head meets its maximum at the spiked key, after having seen larger-than-zero logits before it
        am = R.probabilities(R.late_spike(B, S, C_, heads, pos), heads).argmax(-1)
        assert ((am == pos).sum(-1) > 0).all()


def test_spike_positions_cover_the_late_paths():
    assert R.spike_positions(17) == [16]
    assert R.spike_positions(64) == [48, 50, 63]                      # 48 .. 63: the key block of wave 3 when four waves split the keys
    assert R.spike_positions(130) == [50, 128, 129]
    assert R.spike_positions(1040) == [50, 128, 1024, 1039]


def test_poisoned_surround_detects_writes():
    p = R.Poisoned((3, 5), "cpu", torch.ones(3, 5))
    assert p.surround_unchanged() and torch.equal(p.t, torch.ones(3, 5)) and p.buf.isnan().sum() == 2 * R.Poisoned.PAD
    p.buf[R.Poisoned.PAD + 14] = 2.0
    assert p.surround_unchanged() and p.t[2, 4] == 2.0
    p.buf[R.Poisoned.PAD + 15] = 0.0
    assert not p.surround_unchanged()
    p = R.Poisoned((4,), "cpu")
    p.buf[R.Poisoned.PAD - 1] = float("nan")                         # the same NaN again is no change
    assert p.surround_unchanged() and p.t.isnan().all()


# ---- the tables against the dispatch ---------------------------------------------------------------------------------------------
def test_forward_table_matches_dispatch_and_reaches_every_variant():
    lib = N.lib()
    assert lib.sbgm_abi_version() == N.ABI_VERSION >= 8              # the queries came with version 8
    n = lib.sbgm_mha_core_fwd_variant_count()
    names = [lib.sbgm_mha_core_fwd_variant_name(i).decode() for i in range(n)]
    assert n == 29 and len(set(names)) == n and lib.sbgm_mha_core_fwd_variant_name(n) is None
    assert lib.sbgm_mha_core_fwd_variant_name(-1) is None
    reached = set()
    for B, S, C_, heads, expect in T.FWD:
        vid, info = fwd_query(B, S, C_, heads)
        if expect == T.REFUSED:
            assert vid == -1, (B, S, C_, heads, vid)
            continue
        assert vid >= 0, f"{(B, S, C_, heads)} is refused but the table does not say so"
        assert info[:3] == expect, ((B, S, C_, heads), info, expect)
        fam, d16, kn = expect
        assert names[vid] == f"{'mha_core_lds_kernel' if fam == T.LDS else 'mha_core_kernel'}<{d16},{kn}>"
        reached.add(vid)
    assert reached == set(range(n)), "unreached: " + ", ".join(names[i] for i in sorted(set(range(n)) - reached))


def test_forward_table_hits_the_launch_geometries_it_claims():
    """per_wave 4 with a ragged last slot, per_wave 3 with an empty slot, the two-workgroups-per-CU rule"""
    def geometry(B, S, C_, heads):
        _, (_, _, nq, qsplit) = fwd_query(B, S, C_, heads)
        return nq, qsplit, ((S + 15) // 16 + 4 * qsplit - 1) // (4 * qsplit)
    assert geometry(16, 200, 256, 16) == (4, 1, 4) and geometry(16, 192, 128, 16) == (4, 1, 3)
    assert geometry(8, 136, 128, 16) == (2, 2, 2)
    assert geometry(1, 1040, 32, 1) == (1, 65, 1) and geometry(1, 130, 64, 2) == (1, 9, 1)
    assert geometry(32, 256, 128, 8)[0] == 4                           # a batch-32 sampling run: the variant the table's NQ = 4 shapes stand for


def test_forward_head_dims():
    """every head dim the reference's configurations produce is served; the refused ones are exactly those whose d16 has no kernel"""
    for C_ in T.REFERENCE_CHANNELS:
        for heads in T.REFERENCE_HEADS:
            for S in (16, 64, 256, 1024):
                assert fwd_query(8, S, C_, heads)[0] >= 0, (C_, heads, S)
    served16 = {1, 2, 3, 4, 6, 8, 12, 16, 32}
    for d in range(1, 530):
        for S in (17, 130):
            vid, _ = fwd_query(1, S, d, 1)
            assert (vid >= 0) == (d % 4 == 0 and (d + 15) // 16 in served16), (d, S, vid)
    assert fwd_query(1, 17, 64, 3)[0] == -1 and fwd_query(0, 17, 64, 2)[0] == -1 and fwd_query(1, 0, 64, 2)[0] == -1


def test_backward_table_matches_dispatch_and_reaches_every_variant():
    lib = N.lib()
    n = lib.sbgm_mha_core_bwd_variant_count()
    names = [lib.sbgm_mha_core_bwd_variant_name(i).decode() for i in range(n)]
    assert names == ["mha_core_bwd_mfma_kernel<32>", "mha_core_bwd_mfma_kernel<64>", "mha_core_bwd_mfma_kernel<128>",
                     "mha_core_bwd_lds_kernel<16>", "mha_core_bwd_lds_kernel<32>", "mha_core_bwd_kernel"]
    assert lib.sbgm_mha_core_bwd_variant_name(n) is None
    reached, groups = set(), set()
    for B, S, C_, heads, expect in T.BWD:
        vid, info = bwd_query(B, S, C_, heads)
        if expect == T.REFUSED:
            assert vid == -1, (B, S, C_, heads, vid)
            continue
        assert vid >= 0, f"{(B, S, C_, heads)} is refused but the table does not say so"
        assert info[:3] == expect, ((B, S, C_, heads), info, expect)
        qblocks, G = (S + 15) // 16, info[2]
        assert info[3] == B * heads * ((qblocks + G - 1) // G)
        reached.add(vid)
        if expect[0] == T.MFMA:
            groups.add((expect[1], G > 1, qblocks % G != 0))
    assert reached == set(range(n))
    for d in (32, 64, 128):                                            # each matrix-pipe head dim alone and with several blocks per workgroup
        assert (d, False, False) in groups and (d, True, False) in groups
    assert (32, True, True) in groups and (64, True, True) in groups   # ragged last group
    assert bwd_query(1, 1200, 32, 1)[0] >= 0 and bwd_query(1, 16, 64, 3)[0] == -1


def test_token_table_matches_dispatch_and_reaches_every_variant():
    lib = N.lib()
    n = lib.sbgm_attn_tokens_variant_count()
    names = [lib.sbgm_attn_tokens_variant_name(i).decode() for i in range(n)]
    assert n == 8 and len(set(names)) == n and lib.sbgm_attn_tokens_variant_name(n) is None
    reached = set()
    for M, C_, expect in T.TOKENS:
        vid, info = tok_query(M, C_)
        if expect == T.REFUSED:
            assert vid == -1, (M, C_, vid)
            continue
        assert vid >= 0 and info == expect, ((M, C_), vid, info, expect)
        assert names[vid] == "attn_in_kernel<{0},{1}>, attn_out_kernel<{0},{1}>".format(expect[0], expect[1] // 16)
        reached.add(vid)
    assert reached == set(range(n))
    assert tok_query(0, 64)[0] == -1 and tok_query(16383, 64)[1][1] == 16 and tok_query(16384, 64)[1][1] == 32
