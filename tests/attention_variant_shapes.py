"""Shape tables of tests/test_gpu_attention_variants.py: the smallest shapes that reach every kernel instantiation behind
sbgm_mha_core_fwd, sbgm_mha_core_bwd and sbgm_attn_qkv_fwd / sbgm_attn_tail_fwd.

Each entry states what the launcher must pick for it; tests/test_cpu_attention_variants.py asks the library's own dispatch
(sbgm_*_variant, no device needed) and fails if an entry is wrong, if an instantiation is reached by no entry, or if a refused
shape is not listed as REFUSED.
"""
REFUSED = "refused"
REG, LDS = 0, 1                                   # _native.MHA_FWD_*
MFMA, LDS16, LDS32, SCALAR = 0, 1, 2, 3           # _native.MHA_BWD_*


def _fwd(B, S, d, heads, expect):
    return (B, S, d * heads, heads, expect)


# (B, S, C, heads, (family, d16, KSPLIT | NQ) | REFUSED)
FWD = (
    # register kernel, KSPLIT = 1 (S < 64): every d16, full and partial last 16-block, two samples x two heads = two workgroups
    [_fwd(2, 17, d, 2, (REG, (d + 15) // 16, 1)) for d in (8, 16, 20, 32, 48, 64, 96, 128, 192, 256, 512)] +
    # head dim 512 never splits its keys and never takes the LDS kernel
    [_fwd(1, 130, 512, 1, (REG, 32, 1))] +
    # register kernel, KSPLIT = 4: exactly one key block per wave, one key in a fifth block, ragged last block
    [_fwd(2, S, d, 2, (REG, (d + 15) // 16, 4)) for d in (8, 16, 20, 32, 48, 64) for S in (64, 65, 127)] +
    # ... and the head dims that bypass the LDS kernel at S >= 128
    [_fwd(1, 130, d, 2, (REG, d // 16, 4)) for d in (96, 128, 192, 256)] +
    # LDS kernel, one query block per wave: one full chunk, one key / two keys in the second chunk
    [_fwd(1, S, d, 2, (LDS, (d + 15) // 16, 1)) for d in (16, 32, 48, 64) for S in (128, 129, 130)] +
    [_fwd(1, 129, 20, 2, (LDS, 2, 1))] +
    [_fwd(1, 1040, 32, 1, (LDS, 2, 1))] +          # S >= 1024: two workgroups per CU, nine chunks
    # LDS kernel, two query blocks per wave (128 heads, 9 query blocks over 2 workgroups), ragged S
    [_fwd(8, 136, d, 16, (LDS, (d + 15) // 16, 2)) for d in (8, 20, 48, 64)] +
    # LDS kernel, four query blocks per wave (256 heads, qsplit 1): 13 blocks = the last wave slot ragged, 12 blocks = one slot empty
    [_fwd(16, 200, d, 16, (LDS, (d + 15) // 16, 4)) for d in (16, 32, 48, 64)] +
    [_fwd(16, 192, d, 16, (LDS, (d + 15) // 16, 4)) for d in (8, 20, 40, 64)] +
    # head dims whose d16 has no instantiation
    [_fwd(1, 17, d, 1, REFUSED) for d in (80, 100)] + [_fwd(1, 130, 80, 1, REFUSED)]
)


def _bwd(B, S, d, heads, expect):
    return (B, S, d * heads, heads, expect)


# (B, S, C, heads, (family, head dim, G) | REFUSED)
BWD = [
    # matrix-pipe kernel, G = 1: the longest S of each head dim, one past it (the staged kernel), and short ragged ones
    _bwd(1, 256, 32, 2, (MFMA, 32, 1)), _bwd(1, 257, 32, 2, (LDS32, 32, 1)), _bwd(2, 40, 32, 2, (MFMA, 32, 1)),
    _bwd(1, 128, 64, 2, (MFMA, 64, 1)), _bwd(1, 129, 64, 2, (LDS32, 64, 1)), _bwd(2, 17, 64, 2, (MFMA, 64, 1)),
    _bwd(1, 64, 128, 2, (MFMA, 128, 1)), _bwd(1, 65, 128, 2, (LDS32, 128, 1)), _bwd(2, 33, 128, 2, (MFMA, 128, 1)),
    _bwd(2, 4, 32, 2, (MFMA, 32, 1)),                                # S < 16 with a matrix-pipe head dim stays on the matrix pipe
    # G = 2: 512 query blocks in all
    _bwd(8, 256, 32, 4, (MFMA, 32, 2)), _bwd(8, 128, 64, 8, (MFMA, 64, 2)), _bwd(16, 64, 128, 8, (MFMA, 128, 2)),
    # ragged last group: 9 blocks in groups of 2; 8 blocks in groups of 3 with a ragged last block
    _bwd(8, 144, 32, 8, (MFMA, 32, 2)), _bwd(12, 120, 64, 8, (MFMA, 64, 3)),
    # staged kernel with 16 lanes per query (S < 16) and 32
    _bwd(2, 4, 8, 2, (LDS16, 8, 1)), _bwd(2, 15, 8, 2, (LDS16, 8, 1)), _bwd(2, 4, 16, 2, (LDS16, 16, 1)),
    _bwd(2, 15, 16, 2, (LDS16, 16, 1)), _bwd(1, 144, 12, 2, (LDS32, 12, 1)), _bwd(2, 16, 8, 2, (LDS32, 8, 1)),
    # scalar kernel: K / V too large for LDS; a head dim that is no multiple of 4 (this launcher does not refuse it)
    _bwd(1, 1024, 32, 1, (SCALAR, 32, 1)), _bwd(2, 20, 6, 2, (SCALAR, 6, 1)),
    # the score rows of 16 queries no longer fit the LDS
    _bwd(1, 1201, 32, 1, REFUSED),
]

# (M, C, (C / 64, tile tokens) | REFUSED): 32-token tiles from M = 16384 (last tile full, one token, half), 16-token tiles below
TOKENS = [(M, C, (C // 64, 32 if M >= 16384 else 16)) for C in (64, 128, 256, 512) for M in (4096, 16383, 16384, 16385, 16400)] + \
         [(16384, 96, REFUSED), (100, 1024, REFUSED)]

# what the reference's configurations can ask of the forward kernel: its attention blocks have 64 .. 512 channels (the encoder
# always ends at 512) and its sweep draws num_heads from (1, 2, 4, 8, 16)
REFERENCE_CHANNELS, REFERENCE_HEADS = (64, 128, 256, 512), (1, 2, 4, 8, 16)
