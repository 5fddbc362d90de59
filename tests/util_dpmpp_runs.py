"""dpmpp_2m_sampler runs in a fresh interpreter, for the switch the library reads once per process (SBGM_NO_TIME_ROWS); follows
tests/util_step_runs.py: `run_specs(specs, env, path)` starts ONE child that runs every spec in order on the smallest network input
(32 x 32, `build_pair` weights) and returns {spec name: the samples as a numpy array}.

A spec is a dict: name; B; N (steps); and optionally eta, classes (the model has a label embedding), labels (pass a label vector),
guided, held, joint (two overlapping tiles of a 32 x 48 domain; B is then 2), graph (default True), seed."""
import json
import os
import subprocess
import sys

import numpy as np

from util_step_runs import GUIDED, HW, ROOT, SWITCHES


def _child(specs, out_path):
    import torch
    import sbgm_danra_amd as S
    from sbgm_danra_amd.tiling import FullDomainTiler
    from util_models import build_pair

    nets, out = {}, {}
    for sp in specs:
        classes, B = sp.get("classes"), sp["B"]
        if classes not in nets:
            nets[classes] = build_pair(1, classes)[1].eval()
        g = torch.Generator().manual_seed(200 + B)
        kw = dict(batch_size=B, num_steps=sp["N"], device="cuda", img_size=HW, seed=sp.get("seed", 5), use_graph=sp.get("graph", True),
                  eta=sp.get("eta", 0.0))
        if sp.get("joint"):
            t = FullDomainTiler((HW, 48), HW, 8)
            assert len(t) == B == 2
            kw.update(cond_img=t.extract(torch.randn(1, HW, 48, generator=g).cuda()), tile_origins=t.origins_dev, domain_width=t.Wd_pad,
                      joint_tiles=(t.Hd, t.overlap))
        else:
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
            res = S.dpmpp_2m_sampler(nets[classes], S.marginal_prob_std_fn, S.diffusion_coeff_fn, **kw)
        torch.cuda.synchronize()
        out[sp["name"]] = res.cpu().numpy()
    np.savez(out_path, **out)


def run_specs(specs, env, path, timeout=600):
    """one child interpreter with `env` laid over the caller's environment minus the switches; its exit status is checked"""
    base = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    code = ("import json, sys; sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + '/tests'); "
            "import util_dpmpp_runs as U; U._child(json.loads(sys.argv[2]), sys.argv[3])")
    r = subprocess.run([sys.executable, "-c", code, ROOT, json.dumps(specs), str(path)], env=dict(base, **env), capture_output=True,
                       text=True, timeout=timeout)
    assert r.returncode == 0, r.stderr[-3000:]
    with np.load(str(path)) as z:
        return {k: z[k] for k in z.files}
