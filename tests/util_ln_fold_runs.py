"""One 64 x 64 network (build_pair weights, one condition channel, batch 2) in a fresh interpreter, for SBGM_NO_LN_FOLD, which the
library reads once per process: `run(env, path)` starts a child that evaluates the network through sbgm_model_profile_forward (the
measuring route: the fold where the switch allows it), through the plain forward (never folded), and as a 3-step Euler-Maruyama run on
given noise, graph replay and eager launches, and returns the arrays.  `inputs()` are the seeded inputs both sides use.

`python tests/util_ln_fold_runs.py ROOT OUT` runs the child on the package under ROOT (the fixture of the parent commit's samples,
tests/golden/ln_fold_parent_64.npz, was written that way from the parent's tree)."""
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SWITCH = "SBGM_NO_LN_FOLD"
B, HW, STEPS = 2, 64, 3


def inputs():
    import torch
    g = torch.Generator().manual_seed(1406)
    x, c = torch.randn(B, 1, HW, HW, generator=g), torch.randn(B, 1, HW, HW, generator=g)
    t = torch.rand(B, generator=g) * 0.9 + 0.05
    noise = [torch.randn(B, 1, HW, HW, generator=g) for _ in range(STEPS + 1)]
    return x, c, t, noise


def _child(out_path):
    import ctypes as C
    import torch
    import sbgm_danra_amd as S
    from sbgm_danra_amd import _native as N
    from util_models import build_pair

    net = build_pair(1)[1].eval()
    x, c, t, noise = inputs()
    xd, cd, td = x.cuda(), c.cuda(), t.cuda()
    out = {}
    with torch.no_grad():
        out["plain"] = net(xd, td, cond_img=cd).cpu().numpy()
        eng = net._engine(None, None, cd)
        prof, o = N.Profile(), torch.empty_like(xd)
        csv_path = out_path + ".csv"
        N.check(N.lib().sbgm_model_profile_forward(eng.h, xd.data_ptr(), td.data_ptr(), None, cd.data_ptr(), None, None, o.data_ptr(), B, HW, HW,
                                                   C.byref(prof), csv_path.encode(), N.stream()))
        torch.cuda.synchronize()
        out["measured"] = o.cpu().numpy()
        out["kernels"] = np.array([ln.rsplit(",", 1)[1].strip() for ln in open(csv_path).read().splitlines()[1:]])
        kw = dict(batch_size=B, num_steps=STEPS, device="cuda", img_size=HW, cond_img=cd, noise=noise)
        for name, graph in (("em_graph", True), ("em_eager", False), ("em_graph_again", True)):
            out[name] = S.Euler_Maruyama_sampler(net, S.marginal_prob_std_fn, S.diffusion_coeff_fn, use_graph=graph, **kw).cpu().numpy()
        out["plain_after"] = net(xd, td, cond_img=cd).cpu().numpy()
    np.savez(out_path, **out)


def run(env, path, timeout=600):
    base = {k: v for k, v in os.environ.items() if k != SWITCH}
    r = subprocess.run([sys.executable, os.path.abspath(__file__), ROOT, str(path)], env=dict(base, **env), capture_output=True, text=True,
                       timeout=timeout)
    assert r.returncode == 0, r.stderr[-3000:]
    with np.load(str(path)) as z:
        return {k: z[k] for k in z.files}


if __name__ == "__main__":
    sys.path.insert(0, sys.argv[1])
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    _child(sys.argv[2])
