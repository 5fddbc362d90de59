"""The folded LayerNorms inside a whole 64 x 64 network: sbgm_model_profile_forward and a 3-step Euler-Maruyama run with and without
SBGM_NO_LN_FOLD (two fresh interpreters, tests/util_ln_fold_runs.py), both measured against the float64 oracle chain.

 * the fold's error against float64 is at most twice the switch's error on the same inputs (evaluation and run);
 * with the switch set the outputs are bitwise those of the parent commit (tests/golden/ln_fold_parent_64.npz, written by the same
   child from the parent's tree);
 * graph replay equals eager launches bit for bit on the route, and a second run replays the cached graph to the same bits;
 * the plain forward does not take the route: same bits with and without the switch, before and after a run;
 * the profile names the nine-argument kernel for the eight folded linears and the eight-argument one for the rest.

Last, a measurement (no pass / fail line beyond finiteness): the largest |mean|/sigma of the rows entering ln1 / ln2 of the three
deep blocks under the benchmark's initialisation, which says how far the network's rows are from the conditioning the kernel bound
scales with."""
import os

import numpy as np
import pytest
import torch

import util_ln_fold_runs as U

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ln_fold_parent_64.npz")


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    d = tmp_path_factory.mktemp("ln_fold")
    return {"fold": U.run({}, d / "fold.npz"), "switch": U.run({U.SWITCH: "1"}, d / "switch.npz")}


@pytest.fixture(scope="module")
def oracle64():
    """the float64 chain: one evaluation and the 3-step run on the child's inputs"""
    from oracle import torch_ref as O
    ora = O.build_scorenet(1)                      # the oracle of util_models.build_pair(1), which the child runs natively
    ora.load_state_dict(O.synth_state_dict(ora))
    ora = ora.double().eval()
    x, c, t, noise = U.inputs()
    torch.set_default_dtype(torch.float64)
    try:
        with torch.no_grad():
            fwd = ora(x.double(), t.double(), cond_img=c.double())
            em = O.Euler_Maruyama_sampler(ora, O.marginal_prob_std_fn, O.diffusion_coeff_fn, batch_size=U.B, num_steps=U.STEPS, device="cpu",
                                          cond_img=c.double(), noise=iter(n.double() for n in noise), init_hw=U.HW)
    finally:
        torch.set_default_dtype(torch.float32)
    return {"measured": fwd.numpy(), "em_graph": em.numpy()}


def rel(a, b):
    return float(np.abs(a.astype(np.float64) - b).max() / np.abs(b).max())


@pytest.mark.parametrize("what", ["measured", "em_graph"])
def test_fold_error_against_float64_is_at_most_twice_the_switchs(runs, oracle64, what):
    e_fold, e_switch = rel(runs["fold"][what], oracle64[what]), rel(runs["switch"][what], oracle64[what])
    diff = rel(runs["fold"][what], runs["switch"][what].astype(np.float64))
    print(f"LN-FOLD-NET {what}: error against float64 with the fold {e_fold:.3e}, with SBGM_NO_LN_FOLD=1 {e_switch:.3e}; "
          f"fold against switch {diff:.3e} of max|x|")
    assert np.isfinite(runs["fold"][what]).all()
    assert e_fold <= 2 * e_switch


def test_switch_restores_the_parents_bits(runs):
    with np.load(GOLDEN) as z:
        for k in ("plain", "measured", "em_graph", "em_eager"):
            assert np.array_equal(runs["switch"][k], z[k]), k


def test_graph_replay_equals_eager_launches_on_the_route(runs):
    for name in ("fold", "switch"):
        r = runs[name]
        assert np.array_equal(r["em_graph"], r["em_eager"]), name
        assert np.array_equal(r["em_graph"], r["em_graph_again"]), name
    assert not np.array_equal(runs["fold"]["em_graph"], runs["switch"]["em_graph"]), "the run did not take the folded route"


def test_plain_forward_keeps_the_two_launches(runs):
    assert np.array_equal(runs["fold"]["plain"], runs["switch"]["plain"])
    assert np.array_equal(runs["fold"]["plain"], runs["fold"]["plain_after"])
    assert not np.array_equal(runs["fold"]["measured"], runs["switch"]["measured"]), "the measuring route did not fold"


def test_profile_names_the_folded_kernels(runs):
    """64 x 64, batch 2: all four attention blocks run separate GEMMs (32, 8, 32 and 512 tokens), two folded linears each"""
    folded = [k for k in runs["fold"]["kernels"] if k.startswith("conv_igemm_kernel<1; 1; 1; 0; 1; ")]
    assert len(folded) == 8, list(runs["fold"]["kernels"])
    assert not [k for k in runs["switch"]["kernels"] if k.startswith("conv_igemm_kernel<1; 1; 1; 0; 1; ")]
    assert len(runs["fold"]["kernels"]) == len(runs["switch"]["kernels"])


def test_tile_table_rows_of_the_folded_launch(tmp_path):
    """in_mode 3 rows load on the 1x1 / stride 1 implicit-GEMM geometry only: any other geometry, family, grid split-K or a tap
    projection is refused on load and leaves the table as it was; a loaded row is the tile the profile then names"""
    import csv
    import ctypes as C
    from sbgm_danra_amd import _native as N
    from util_models import build_pair
    net = build_pair(1)[1].eval()
    x, c, t, _ = U.inputs()
    xd, cd, td = x.cuda(), c.cuda(), t.cuda()
    eng = net._engine(None, None, cd)
    good = "1 1 1 0 1 1 32 256 768 0 3 | 1 2 1 4 0 0\n"            # in_proj of the 4x4-map block at batch 2: 32 tokens x 256 channels
    bad = ["3 3 1 1 2 16 16 64 64 0 3 | 2 1 1 1 0 0\n",            # a 3x3 convolution
           "1 1 2 0 2 16 16 64 128 0 3 | 2 1 1 1 0 0\n",           # stride 2
           "1 1 1 0 1 1 32 256 768 0 3 | 2 1 2 1 0 0\n",           # grid split-K
           "1 1 1 0 1 1 32 256 768 0 3 | 2 1 1 1 1 0\n",           # a Winograd family
           "1 1 1 0 1 1 32 256 768 1 3 | 2 1 1 1 0 0\n",           # tap projection
           "1 1 1 0 1 1 32 8 768 0 3 | 2 1 1 1 0 0\n",             # fewer than 16 channels
           "1 1 1 0 1 1 32 256 768 0 4 | 2 1 1 1 0 0\n"]           # no such mode
    for i, row in enumerate(bad):
        path = tmp_path / f"bad{i}.txt"
        path.write_text("# sbgm conv tile table v2\n" + row)
        with pytest.raises(N.NativeError, match="malformed"):
            N.check(eng.lib.sbgm_model_tune_load(eng.h, os.fsencode(str(path))))
    path = tmp_path / "good.txt"
    path.write_text("# sbgm conv tile table v2\n" + good)
    N.check(eng.lib.sbgm_model_tune_load(eng.h, os.fsencode(str(path))))
    saved = tmp_path / "saved.txt"
    N.check(eng.lib.sbgm_model_tune_save(eng.h, os.fsencode(str(saved))))
    assert saved.read_text() == "# sbgm conv tile table v2\n" + good
    prof, o, rows = N.Profile(), torch.empty_like(xd), str(tmp_path / "convs.csv")
    N.check(eng.lib.sbgm_model_profile_forward(eng.h, xd.data_ptr(), td.data_ptr(), None, cd.data_ptr(), None, None, o.data_ptr(), U.B, U.HW, U.HW,
                                               C.byref(prof), rows.encode(), N.stream()))
    torch.cuda.synchronize()
    hit = [r["kernel"] for r in csv.DictReader(open(rows)) if (r["kh"], r["W"], r["Cin_pad"], r["Cout"]) == ("1", "32", "256", "768")]
    assert "conv_igemm_kernel<1; 1; 1; 0; 1; 1; 2; 0; 4>" in hit, hit
    assert torch.isfinite(o).all()


def test_rows_of_the_deep_blocks_under_the_benchmarks_initialisation():
    """Measurement: |mean|/sigma of the rows entering ln1 / ln2 of every attention block (the oracle's modules on the weights of
    bench.build_model, hooks on the LayerNorms; 128 x 128, batch 2), tied to the native network by its last feature map."""
    import bench
    from oracle import torch_ref as O
    net = bench.build_model(torch.device("cuda"), 1)
    ora = O.build_scorenet(1)
    ora.load_state_dict({k: v.cpu() for k, v in net.state_dict().items()})
    ora.eval()
    seen = {}

    def hook(name):
        def f(mod, args):
            rows = args[0].detach().double().reshape(-1, args[0].shape[-1])
            ratio = rows.mean(1).abs() / rows.std(1, unbiased=False).clamp_min(1e-30)
            seen[name] = (tuple(rows.shape), float(ratio.max()), float(ratio.median()))
        return f

    for name, mod in ora.named_modules():
        if isinstance(mod, torch.nn.LayerNorm):
            mod.register_forward_pre_hook(hook(name))
    g = torch.Generator().manual_seed(42)
    x, c = torch.randn(2, 1, 128, 128, generator=g), torch.randn(2, 1, 128, 128, generator=g)
    t = torch.rand(2, generator=g) * 0.9 + 0.05
    fm = []
    with torch.no_grad():
        want = ora(x, t, cond_img=c)
        got = net(x.cuda(), t.cuda(), cond_img=c.cuda(), _fmaps=fm).cpu()
    print(f"LN-FOLD-ROWS native against oracle: {float((got - want).abs().max() / want.abs().max()):.3e}")
    assert seen and torch.isfinite(got).all() and float((got - want).abs().max() / want.abs().max()) <= 1e-4
    for name, (shape, worst, med) in sorted(seen.items()):
        print(f"LN-FOLD-ROWS {name}: rows {shape} max |mean|/sigma = {worst:.3f}, median {med:.3f}")
