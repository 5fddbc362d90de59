"""Speed probe of rk45_sampler (native loop, captured attempt) against the scipy-driven ode_sampler, one JSON line.

At (B = 2, 32 x 32, no condition) and at the C2 shape (B = 32, 128 x 128, one low-res condition; ode_sampler itself passes no condition,
so there it is given the network closed over the same condition field) both samplers solve the same problem: same model, same start z,
same tolerances.  They are timed alternately in one process, after one warm-up run each (workspace sizing, graph capture); every timing
ends in a device synchronise.  Reported per shape: evaluations that counted, wall time per run (median of --reps) and ms per counted
evaluation for both, their ratio, and the native figure again from runs that follow each other directly, per counted and per
executed evaluation (a run executes one surplus attempt of six evaluations after its last step).  Eval mode, no autotune.

Usage: python tools/ode_sampler_speed.py [--tol 1e-3] [--reps 3] [--shapes 2x32,32x128]"""
import argparse
import json
import os
import statistics
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


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def probe(B, HW, tol, reps, max_steps):
    n_cond = 0 if HW < 64 else 1
    torch.manual_seed(0)                                           # the same weights, hence the same steps, in every run
    net = build(n_cond)
    g = torch.Generator().manual_seed(1)
    cond = torch.randn(B, 1, HW, HW, generator=g).cuda() if n_cond else None
    z = (torch.randn(B, 1, HW, HW, generator=g) * float(S.marginal_prob_std_fn(torch.ones(1))[0])).cuda()
    fns = (S.marginal_prob_std_fn, S.diffusion_coeff_fn)
    closed = net if cond is None else (lambda x, t: net(x, t, cond_img=cond))
    native = lambda: S.rk45_sampler(net, *fns, z=z, cond_img=cond, rtol=tol, atol=tol, max_steps=max_steps, return_stats=True)  # noqa: E731
    scipy_ = lambda: S.ode_sampler(closed, *fns, batch_size=B, device="cuda", z=z, atol=tol, rtol=tol, return_nfev=True)  # noqa: E731
    timed(native), timed(scipy_)                                   # warm-up
    tn, ts = [], []
    for _ in range(reps):                                          # alternately, so drift hits both alike
        t, (xn, st) = timed(native)
        tn.append(t)
        t, (xs, nfev_s) = timed(scipy_)
        ts.append(t)
    tb = statistics.median(timed(native)[0] for _ in range(reps))  # back to back: no mostly idle scipy run in between
    tn_, ts_ = statistics.median(tn), statistics.median(ts)
    nfev_n = int(st["nfev"])
    return {"shape": {"B": B, "H": HW, "W": HW, "n_cond": n_cond}, "tol": tol, "reps": reps,
            "rk45_nfev": nfev_n, "rk45_accepted": int(st["n_accepted"]), "rk45_rejected": int(st["n_rejected"]),
            "rk45_surplus_attempts": int(st["surplus_attempts"]), "rk45_s_per_run": round(tn_, 5),
            "rk45_ms_per_eval": round(tn_ / nfev_n * 1e3, 4),
            "rk45_ms_per_eval_back_to_back": round(tb / nfev_n * 1e3, 4),
            "rk45_ms_per_executed_eval_back_to_back": round(tb / (nfev_n + 6 * int(st["surplus_attempts"])) * 1e3, 4),
            "scipy_nfev": int(nfev_s), "scipy_s_per_run": round(ts_, 5), "scipy_ms_per_eval": round(ts_ / int(nfev_s) * 1e3, 4),
            "scipy_over_rk45_per_eval": round((ts_ / int(nfev_s)) / (tn_ / nfev_n), 3),
            "max_rel_diff": float((xn.double() - xs).abs().max() / xs.abs().max()),
            "finite": bool(torch.isfinite(xn).all() and torch.isfinite(xs).all())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tol", type=float, default=1e-3)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--max-steps", type=int, default=2000)
    ap.add_argument("--shapes", default="2x32,32x128", help="comma-separated BxHW")
    a = ap.parse_args()
    shapes = [tuple(int(v) for v in s.split("x")) for s in a.shapes.split(",")]
    print(json.dumps({"probes": [probe(B, HW, a.tol, a.reps, a.max_steps) for B, HW in shapes]}), flush=True)


if __name__ == "__main__":
    main()
