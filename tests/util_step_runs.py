"""Sampler runs in a fresh interpreter, for switches the library reads once per process (SBGM_NO_TIME_ROWS, SBGM_NO_CONV_PAIR):
`run_specs(specs, env, path)` starts one child that runs every spec in order on the smallest network input (32 x 32, `build_pair`
weights) and returns {spec name: the samples as a numpy array}.

A spec is a dict: name; kind (default "dpm"); B; N (steps); and optionally n_cond (condition channels of the model, default 1: one
cond_img channel; 0: none), classes (the model has a label embedding), labels (pass a label vector), guided, held, joint (two
overlapping tiles of a 32 x 48 domain; B is then 2), graph (default True), eps, seed, fresh (build a new model instead of the child's
cached one of that kind: a new engine handle), ws (also return the engine's sbgm_model_workspace_bytes after the case, as `<name>/ws`).

The kinds: "em" | "pc"; "edm" (EDM Heun, optionally s_churn); "dpm" (DPM-Solver++(2M), optionally eta); "rk45" (optionally rtol = atol,
default 1e-2; the solver's integer statistics nfev, accepted, rejected, surplus attempts come back as `<name>/stats`); "forward" (one
plain evaluation instead of a run); "measured" (one sbgm_model_profile_forward evaluation; the kernel-name column of its CSV comes back
as `<name>/kernels`)."""
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUIDED = {"classifier_free_guidance": {"enabled": True, "guidance_scale": 2.5, "guidance_scale_max": 1.5}}
SWITCHES = ("SBGM_NO_TIME_ROWS", "SBGM_NO_CONV_PAIR")
HW = 32


def _child(specs, out_path):
    import ctypes as C
    import torch
    import sbgm_danra_amd as S
    from sbgm_danra_amd import _native as N
    from sbgm_danra_amd.tiling import FullDomainTiler
    from util_models import build_pair

    nets = {}

    def model(n_cond, classes, fresh):
        key = (n_cond, classes)
        if fresh or key not in nets:
            net = build_pair(n_cond, classes)[1].eval()
            if fresh:
                return net
            nets[key] = net
        return nets[key]

    out = {}
    for sp in specs:
        n_cond, classes, B = sp.get("n_cond", 1), sp.get("classes"), sp["B"]
        net = model(n_cond, classes, sp.get("fresh", False))
        kind = sp.get("kind", "dpm")
        g = torch.Generator().manual_seed(200 + B if kind == "dpm" else 100 + B + n_cond)
        kw = dict(batch_size=B, num_steps=sp["N"], device="cuda", img_size=HW, seed=sp.get("seed", 5), eps=sp.get("eps", 1e-3),
                  use_graph=sp.get("graph", True))
        if sp.get("joint"):
            t = FullDomainTiler((HW, 48), HW, 8)
            assert len(t) == B == 2
            kw.update(cond_img=t.extract(torch.randn(1, HW, 48, generator=g).cuda()), tile_origins=t.origins_dev, domain_width=t.Wd_pad,
                      joint_tiles=(t.Hd, t.overlap))
        elif n_cond >= 1:
            kw["cond_img"] = torch.randn(B, 1, HW, HW, generator=g).cuda()
        if sp.get("labels"):
            kw["y"] = torch.randint(0, classes, (B,), generator=g).cuda()
        if sp.get("guided"):
            kw["cfg"] = GUIDED
        if sp.get("held"):
            kw["known"] = torch.randn(B, 1, HW, HW, generator=g).cuda()
            m = torch.zeros(HW, HW)
            m[4:20, 8:24] = 1.0
            m[20:24, 8:24] = 0.5                                   # a soft edge
            kw["known_mask"] = m.cuda()
        with torch.no_grad():
            if kind in ("forward", "measured"):                    # one evaluation instead of a run
                x, t = torch.randn(B, 1, HW, HW, generator=g).cuda(), (torch.rand(B, generator=g) * 0.9 + 0.05).cuda()
                if kind == "forward":
                    res = net(x, t, kw.get("y"), cond_img=kw.get("cond_img"))
                else:
                    res, prof, csv_path = torch.empty_like(x), N.Profile(), str(out_path) + ".csv"
                    N.check(N.lib().sbgm_model_profile_forward(net._engine(None, None, kw.get("cond_img")).h, x.data_ptr(), t.data_ptr(),
                                                               N.ptr(kw.get("y")), N.ptr(kw.get("cond_img")), None, None, res.data_ptr(), B,
                                                               HW, HW, C.byref(prof), csv_path.encode(), N.stream()))
                    torch.cuda.synchronize()
                    out[sp["name"] + "/kernels"] = np.array([ln.rsplit(",", 1)[1].strip() for ln in open(csv_path).read().splitlines()[1:]])
            elif kind == "rk45":
                tol = sp.get("rtol", 1e-2)
                rk = {k: v for k, v in kw.items() if k != "num_steps"}
                res, st = S.rk45_sampler(net, S.marginal_prob_std_fn, S.diffusion_coeff_fn, rtol=tol, atol=tol, return_stats=True, **rk)
                out[sp["name"] + "/stats"] = np.array([st["nfev"], st["n_accepted"], st["n_rejected"], st["surplus_attempts"]], dtype=np.int64)
            elif kind == "edm":
                res = S.edm_heun_sampler(net, S.marginal_prob_std_fn, S.diffusion_coeff_fn, s_churn=sp.get("s_churn", 0.0), **kw)
            elif kind == "dpm":
                res = S.dpmpp_2m_sampler(net, S.marginal_prob_std_fn, S.diffusion_coeff_fn, eta=sp.get("eta", 0.0), **kw)
            else:
                fn = S.Euler_Maruyama_sampler if kind == "em" else S.pc_sampler
                res = fn(net, S.marginal_prob_std_fn, S.diffusion_coeff_fn, **kw)
        torch.cuda.synchronize()
        out[sp["name"]] = res.cpu().numpy()
        if sp.get("ws"):
            eng = net._engines[(0, 0, n_cond)]
            out[sp["name"] + "/ws"] = np.int64(N.lib().sbgm_model_workspace_bytes(eng.h))
    np.savez(out_path, **out)


def run_specs(specs, env, path, timeout=600):
    """one child interpreter with `env` laid over the caller's environment minus the switches"""
    base = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    code = ("import json, sys; sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + '/tests'); "
            "import util_step_runs as U; U._child(json.loads(sys.argv[2]), sys.argv[3])")
    r = subprocess.run([sys.executable, "-c", code, ROOT, json.dumps(specs), str(path)], env=dict(base, **env), capture_output=True,
                       text=True, timeout=timeout)
    assert r.returncode == 0, r.stderr[-3000:]
    with np.load(str(path)) as z:
        return {k: z[k] for k in z.files}
