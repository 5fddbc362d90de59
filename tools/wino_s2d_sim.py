"""Numerics of Winograd F(2x2,4x4) for the stem's 8x8 stride-2 convolution run as a 4x4 convolution over the space-to-depth
input (conv_s2w.hip).  Builds A^T, G, B^T for the interpolation points {0, 1, -1, p, inf} exactly (fractions), checks
A^T[(G g) . (B^T d)] == correlation in exact arithmetic, then simulates the kernel's fp32 arithmetic (fp32 input transform,
U = G g G^T rounded once from fp64, sequential fp32 accumulation over K' channels, fp32 output transform) against fp64 and
prints the error relative to each block's largest output.  Usage: python tools/wino_s2d_sim.py [--blocks N] [--channels K]"""
import argparse
from fractions import Fraction as Fr

import numpy as np


def f24_matrices(p4):
    """(AT [2][5], G [5][4], BT [5][5]) as Fractions for the points {0, 1, -1, p4, inf}."""
    pts = [Fr(0), Fr(1), Fr(-1), Fr(p4)]
    AT = [[pts[j] ** i for j in range(4)] + [Fr(int(i == 1))] for i in range(2)]
    G = []
    for j in range(4):
        n = Fr(1)
        for l in range(4):
            if l != j:
                n *= pts[j] - pts[l]
        G.append([pts[j] ** k / n for k in range(4)])
    G.append([Fr(0), Fr(0), Fr(0), Fr(1)])
    # B^T from  sum_j AT[i][j] G[j][k] BT[j][l] = [l == i + k]: per column l, 8 equations in 5 unknowns (exact elimination)
    BT = [[Fr(0)] * 5 for _ in range(5)]
    for l in range(5):
        rows = [[AT[i][j] * G[j][k] for j in range(5)] + [Fr(int(l == i + k))] for i in range(2) for k in range(4)]
        piv = []
        r = 0
        for c in range(5):
            q = next((q for q in range(r, len(rows)) if rows[q][c] != 0), None)
            if q is None:
                continue
            rows[r], rows[q] = rows[q], rows[r]
            rows[r] = [v / rows[r][c] for v in rows[r]]
            for q in range(len(rows)):
                if q != r and rows[q][c] != 0:
                    f = rows[q][c]
                    rows[q] = [a - f * b for a, b in zip(rows[q], rows[r])]
            piv.append(c)
            r += 1
        assert piv == list(range(5)) and all(all(v == 0 for v in row) for row in rows[5:]), "inconsistent system"
        for j in range(5):
            BT[j][l] = rows[j][5]
    return AT, G, BT


def as_np(m, dt=np.float64):
    return np.array([[float(v) for v in row] for row in m], dtype=dt)


def simulate(p4, blocks, K, seed=0):
    AT, G, BT = (as_np(m) for m in f24_matrices(p4))
    rng = np.random.default_rng(seed)
    d = rng.standard_normal((blocks, K, 5, 5))                   # input tiles (one per channel)
    g = rng.standard_normal((K, 4, 4)) * (1.0 / np.sqrt(K * 16))   # Kaiming-like filter scale
    d32, g32 = d.astype(np.float32), g.astype(np.float32)
    # fp64 reference: direct correlation of the fp32-rounded operands
    ref = np.zeros((blocks, 2, 2))
    for oy in range(2):
        for ox in range(2):
            ref[:, oy, ox] = np.einsum("bkuv,kuv->b", d32[:, :, oy:oy + 4, ox:ox + 4].astype(np.float64), g32.astype(np.float64))
    U = np.einsum("au,kuv,bv->kab", G, g32.astype(np.float64), G).astype(np.float32)
    AT32, BT32 = AT.astype(np.float32), BT.astype(np.float32)
    V = np.einsum("ai,bkij,cj->bkac", BT32, d32, BT32).astype(np.float32)      # fp32 (einsum in fp32)
    M = np.zeros((blocks, 5, 5), dtype=np.float32)
    for k in range(K):                                                          # sequential fp32 accumulation
        M = (M + U[k][None] * V[:, k]).astype(np.float32)
    Y = np.einsum("ia,bac,jc->bij", AT32, M, AT32).astype(np.float32)
    direct = np.zeros((blocks, 2, 2), dtype=np.float32)
    for k in range(K):
        for u in range(4):
            for v in range(4):
                direct = (direct + d32[:, k, u:u + 2, v:v + 2] * g32[k, u, v]).astype(np.float32)
    scale = np.abs(ref).reshape(blocks, -1).max(axis=1)
    ew = (np.abs(Y - ref).reshape(blocks, -1).max(axis=1) / scale)
    ed = (np.abs(direct - ref).reshape(blocks, -1).max(axis=1) / scale)
    return ew, ed


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=40)
    ap.add_argument("--channels", type=int, default=256)
    a = ap.parse_args()
    for p4 in (Fr(2), Fr(-2), Fr(1, 2), Fr(-1, 2)):
        AT, G, BT = f24_matrices(p4)
        ew, ed = simulate(p4, a.blocks, a.channels)
        print(f"p4={str(p4):>5}: winograd median {np.median(ew):.2e} worst {ew.max():.2e} | direct fp32 median {np.median(ed):.2e} "
              f"worst {ed.max():.2e} | max|B^T| {max(abs(float(v)) for r in BT for v in r):g} max|G| {max(abs(float(v)) for r in G for v in r):.3g}")


if __name__ == "__main__":
    main()
