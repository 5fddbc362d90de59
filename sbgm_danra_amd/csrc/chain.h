// The scalar program of sbgm_pointwise_chain as a device function, shared by the post-sampling pass (postproc.hip, K31) and the
// cutout gather (cutout.hip, K49): a chain of separately rounded fp32 tensor-scalar ops in the reference's order (no re-association,
// no FMA contraction), so the affine transforms are bit-identical to the reference and only exp/log differ by the libm implementation.
#pragma once
#include "../../include/sbgm_hip.h"
#include "common.h"

struct ChainProgram {
    int n_ops;
    int op[SBGM_CHAIN_MAX_OPS];
    float c[SBGM_CHAIN_MAX_OPS];
};

__device__ __forceinline__ float chain_apply(float v, const ChainProgram& p) {
#pragma unroll
    for (int i = 0; i < SBGM_CHAIN_MAX_OPS; ++i) {
        if (i >= p.n_ops) break;
        const float c = p.c[i];
        switch (p.op[i]) {
            case SBGM_OP_ADD: v = __fadd_rn(v, c); break;
            case SBGM_OP_MUL: v = __fmul_rn(v, c); break;
            case SBGM_OP_DIV: v = __fdiv_rn(v, c); break;
            case SBGM_OP_CLAMP_MIN: v = v < c ? c : v; break;     // comparisons keep NaN, like torch.clamp
            case SBGM_OP_CLAMP_MAX: v = v > c ? c : v; break;
            case SBGM_OP_EXP: v = expf(v); break;
            case SBGM_OP_LOG: v = logf(v); break;
            default: break;
        }
    }
    return v;
}
