"""Whole-network runs for test_gpu_skip_mix.py in a fresh interpreter (SBGM_NO_SKIP_MIX is read once per process): `run(env, path)`
starts one child that runs a fixed list of cases at 64 x 64, batch 2, on `build_pair` weights and returns {name: numpy array}."""
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SWITCH = "SBGM_NO_SKIP_MIX"
HW, B = 64, 2
GUIDED = {"classifier_free_guidance": {"enabled": True, "guidance_scale": 2.5, "guidance_scale_max": 1.5}}


def _child(out_path):
    import torch
    import sbgm_danra_amd as S
    from sbgm_danra_amd import _native as N
    from util_models import build_pair

    g = torch.Generator().manual_seed(11)
    rn = lambda *s: torch.randn(*s, generator=g).cuda()  # noqa: E731
    c1, c1b, c4 = rn(B, 1, HW, HW), rn(B, 1, HW, HW), rn(B, 4, HW, HW)
    x, t = rn(B, 1, HW, HW), (torch.rand(B, generator=g) * 0.9 + 0.05).cuda()
    fns = (S.marginal_prob_std_fn, S.diffusion_coeff_fn)
    kw = dict(batch_size=B, device="cuda", img_size=HW, seed=5)
    out = {}

    def ws_bytes(net):
        (eng,) = net._engines.values()
        return int(N.lib().sbgm_model_workspace_bytes(eng.h))

    with torch.no_grad():
        net = build_pair(1)[1].eval()
        out["forward"] = net(x, t, cond_img=c1)
        out["ws_forward"] = torch.tensor(ws_bytes(net))
        out["em"] = S.Euler_Maruyama_sampler(net, *fns, num_steps=5, cond_img=c1, **kw)
        # new condition CONTENTS at the same address, straight after: the cached step graph is replayed, so the run's condition share
        # of conv1 must be rebuilt outside it
        c1a = c1.clone()
        c1.copy_(c1b)
        out["em_new_cond"] = S.Euler_Maruyama_sampler(net, *fns, num_steps=5, cond_img=c1, **kw)
        c1.copy_(c1a)
        out["forward_after"] = net(x, t, cond_img=c1)
        out["em_eager"] = S.Euler_Maruyama_sampler(net, *fns, num_steps=5, cond_img=c1, use_graph=False, **kw)
        out["pc"] = S.pc_sampler(net, *fns, num_steps=3, cond_img=c1, **kw)
        out["guided"] = S.Euler_Maruyama_sampler(build_pair(1, 3)[1].eval(), *fns, num_steps=4, cond_img=c1,
                                                 y=torch.tensor([1, 2]).cuda(), cfg=GUIDED, **kw)
        out["cond4"] = S.Euler_Maruyama_sampler(build_pair(4)[1].eval(), *fns, num_steps=4, cond_img=c4, **kw)
        out["nocond"] = S.Euler_Maruyama_sampler(build_pair(0)[1].eval(), *fns, num_steps=4, **kw)
        fresh = build_pair(1)[1].eval()
        out["em_new_cond_fresh"] = S.Euler_Maruyama_sampler(fresh, *fns, num_steps=5, cond_img=c1b, **kw)
        # a model whose first call is a run sizes its workspace for the run (a workspace never shrinks below what an earlier call took:
        # after a plain forward's generous first bound the run's share would not show)
        out["ws_run"] = torch.tensor(ws_bytes(fresh))
        # an upload of conv1.weight between two runs: the packed x weights follow
        net.encoder.conv1.weight.mul_(1.25)
        out["em_new_w1"] = S.Euler_Maruyama_sampler(net, *fns, num_steps=5, cond_img=c1, **kw)
    torch.cuda.synchronize()
    np.savez(out_path, **{k: v.cpu().numpy() for k, v in out.items()})


def run(env, path, timeout=600):
    base = {k: v for k, v in os.environ.items() if k != SWITCH}
    code = ("import sys; sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + '/tests'); "
            "import util_skip_mix_runs as U; U._child(sys.argv[2])")
    r = subprocess.run([sys.executable, "-c", code, ROOT, str(path)], env=dict(base, **env), capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stderr[-3000:]
    with np.load(str(path)) as z:
        return {k: z[k] for k in z.files}
