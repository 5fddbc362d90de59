"""Speed probe of edm_heun_sampler at the C2 shape (B = 32, 128 x 128, one low-res condition, eval mode, no autotune), one JSON line:

* ms per network evaluation of Euler_Maruyama_sampler over 200 steps (after a warm-up run) and of edm_heun_sampler at N = 32
  (63 evaluations, repeated to at least 0.5 s of work); both replay one captured step graph per step, so these should agree;
* wall time per batch of edm_heun_sampler at N = 32 against pc_sampler at 1000 steps (2000 evaluations).

Every timing ends in a device synchronise.  Usage: python tools/edm_sampler_speed.py [--pc-steps 1000] [--edm-steps 32]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
import torch.nn as nn  # noqa: E402

import sbgm_danra_amd as S  # noqa: E402


def build(n_in):
    """a model with the reference's training initialisation (no oracle involved)"""
    enc = S.Encoder(n_in, 256, block_layers=[2, 2, 2, 2], n_heads=4)
    dec = S.Decoder(512, 1, 256, n_heads=4, norm="group", gn_groups=8, activation=nn.SiLU)
    net = S.ScoreNet(S.marginal_prob_std_fn, enc, dec, device=torch.device("cuda"), debug_pre_sigma_div=False)
    with torch.no_grad():
        for m in net.modules():
            if isinstance(m, (nn.Conv2d, nn.ConvTranspose2d)):
                nn.init.xavier_uniform_(m.weight)
                if m.bias is not None:
                    m.bias.fill_(0.01)
    return net.eval()


def timed(fn, reps=1):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--hw", type=int, default=128)
    ap.add_argument("--em-steps", type=int, default=200)
    ap.add_argument("--edm-steps", type=int, default=32)
    ap.add_argument("--pc-steps", type=int, default=1000)
    a = ap.parse_args()
    B, HW = a.batch, a.hw
    net = build(1)
    cond = torch.randn(B, 1, HW, HW, generator=torch.Generator().manual_seed(1)).cuda()
    kw = dict(batch_size=B, device="cuda", img_size=HW, cond_img=cond, seed=1)
    em = lambda n: S.Euler_Maruyama_sampler(net, S.marginal_prob_std_fn, S.diffusion_coeff_fn, num_steps=n, **kw)  # noqa: E731
    edm = lambda: S.edm_heun_sampler(net, S.marginal_prob_std_fn, S.diffusion_coeff_fn, num_steps=a.edm_steps, **kw)  # noqa: E731
    pc = lambda: S.pc_sampler(net, S.marginal_prob_std_fn, S.diffusion_coeff_fn, num_steps=a.pc_steps, **kw)  # noqa: E731

    timed(lambda: em(a.em_steps))                                  # warm-up: workspace sizing, step-graph capture
    t_em, x_em = timed(lambda: em(a.em_steps))
    nfe_edm = 2 * a.edm_steps - 1
    t_one, _ = timed(edm)                                          # warm-up of the EDM step graph
    reps = max(3, int(0.5 / max(t_one, 1e-6)) + 1)
    t_edm, x_edm = timed(edm, reps)
    t_pc, x_pc = timed(pc)
    ms_em = t_em / a.em_steps * 1e3
    ms_edm = t_edm / nfe_edm * 1e3
    print(json.dumps({
        "shape": {"B": B, "H": HW, "W": HW, "n_cond": 1},
        "em_ms_per_eval": round(ms_em, 4), "em_steps": a.em_steps,
        "edm_ms_per_eval": round(ms_edm, 4), "edm_steps": a.edm_steps, "edm_nfe": nfe_edm, "edm_reps": reps,
        "edm_vs_em_per_eval": round(ms_edm / ms_em, 4),
        "edm_s_per_batch": round(t_edm, 4), "pc_s_per_batch": round(t_pc, 4), "pc_steps": a.pc_steps, "pc_nfe": 2 * a.pc_steps,
        "pc_over_edm_wall": round(t_pc / t_edm, 2),
        "finite": bool(torch.isfinite(x_em).all() and torch.isfinite(x_edm).all() and torch.isfinite(x_pc).all()),
    }), flush=True)


if __name__ == "__main__":
    main()
