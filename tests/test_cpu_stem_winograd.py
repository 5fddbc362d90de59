"""The transforms of the space-to-depth Winograd F(2x2,4x4) stem kernel (conv_s2w.hip), in fp64 on the CPU: the 1-D and 2-D
identities A^T[(G g) . (B^T d)] == correlation, and the space-to-depth mapping of the 8x8 stride-2 pad-3 convolution onto a 4x4
stride-1 correlation over cells."""
import torch
import torch.nn.functional as F

# the matrices written out in conv_s2w.hip (points 0, 1, -1, -2, inf)
BT = torch.tensor([[-2, -1, 2, 1, 0],
                   [0, 2, 3, 1, 0],
                   [0, -2, 1, 1, 0],
                   [0, -1, 0, 1, 0],
                   [0, -2, -1, 2, 1]], dtype=torch.float64)
G = torch.tensor([[-1 / 2, 0, 0, 0],
                  [1 / 6, 1 / 6, 1 / 6, 1 / 6],
                  [1 / 2, -1 / 2, 1 / 2, -1 / 2],
                  [-1 / 6, 1 / 3, -2 / 3, 4 / 3],
                  [0, 0, 0, 1]], dtype=torch.float64)
AT = torch.tensor([[1, 1, 1, 1, 0],
                   [0, 1, -1, -2, 1]], dtype=torch.float64)


def test_f2_4_one_dimensional_identity():
    g = torch.Generator().manual_seed(0)
    for _ in range(20):
        d = torch.randn(5, generator=g, dtype=torch.float64)
        w = torch.randn(4, generator=g, dtype=torch.float64)
        y = AT @ ((G @ w) * (BT @ d))
        direct = torch.stack([(w * d[i:i + 4]).sum() for i in range(2)])
        assert torch.allclose(y, direct, rtol=0, atol=1e-12)


def test_f2x2_4x4_two_dimensional_identity():
    g = torch.Generator().manual_seed(1)
    d = torch.randn(64, 5, 5, generator=g, dtype=torch.float64)
    w = torch.randn(64, 4, 4, generator=g, dtype=torch.float64)
    U = G @ w @ G.T
    V = BT @ d @ BT.T
    y = AT @ (U * V) @ AT.T
    direct = F.conv2d(d[:, None], w[:, None], groups=1)                      # [64 tiles][64 filters][2][2]
    want = torch.stack([direct[i, i] for i in range(64)])
    assert torch.allclose(y, want, rtol=0, atol=1e-12)


def test_space_to_depth_mapping_of_the_stride2_pad3_conv():
    """cell c holds input rows 2c - 3 + py (phase py); sub-filter g[u][v] = w[2u + py][2v + px]; the 8x8/s2/p3 convolution equals
    the 4x4 valid correlation over cells o..o+3, and F(2x2,4x4) over 2x2 output blocks reproduces it."""
    g = torch.Generator().manual_seed(2)
    B, Cin, Cout, H, W = 2, 3, 4, 14, 10
    x = torch.randn(B, Cin, H, W, generator=g, dtype=torch.float64)
    w = torch.randn(Cout, Cin, 8, 8, generator=g, dtype=torch.float64)
    want = F.conv2d(x, w, None, 2, 3)
    OH, OW = want.shape[2:]
    xp = F.pad(x, (3, 5, 3, 5))                                              # pixel (r, c) of the image at (r + 3, c + 3)
    cells_y, cells_x = OH + 3 + (OH % 2), OW + 3 + (OW % 2)                  # whole 2x2 blocks
    xp = F.pad(xp, (0, max(0, 2 * cells_x - xp.shape[3]), 0, max(0, 2 * cells_y - xp.shape[2])))
    s2d = torch.stack([xp[:, :, py:2 * cells_y:2, px:2 * cells_x:2] for py in range(2) for px in range(2)], 1)  # [B][4][Cin][cy][cx]
    sub = torch.stack([w[:, :, py::2, px::2] for py in range(2) for px in range(2)], 1)                        # [Cout][4][Cin][4][4]
    direct = F.conv2d(s2d.reshape(B, 4 * Cin, cells_y, cells_x), sub.reshape(Cout, 4 * Cin, 4, 4))
    assert torch.allclose(direct[:, :, :OH, :OW], want, rtol=0, atol=1e-10)
    # Winograd over the 2x2 output blocks of the cell grid
    U = torch.einsum("au,okuv,bv->okab", G, sub.reshape(Cout, 4 * Cin, 4, 4), G)
    got = torch.zeros(B, Cout, cells_y - 3, cells_x - 3, dtype=torch.float64)
    d2 = s2d.reshape(B, 4 * Cin, cells_y, cells_x)
    for by in range(0, cells_y - 3, 2):
        for bx in range(0, cells_x - 3, 2):
            V = torch.einsum("ai,bkij,cj->bkac", BT, d2[:, :, by:by + 5, bx:bx + 5], BT)
            M = torch.einsum("okac,bkac->boac", U, V)
            got[:, :, by:by + 2, bx:bx + 2] = torch.einsum("ia,boac,jc->boij", AT, M, AT)
    assert torch.allclose(got[:, :, :OH, :OW], want, rtol=0, atol=1e-9)
