"""Cost of training.with_ema at the C3 per-GPU training step (128x128, 4 conditions, batch 8): the captured loss + backward replayed,
then the native Adam step with the EMA off (one launch) and on (the same launch with the EMA epilogue + EMA-only descriptors for the
buffers).  Both variants run in the same process on the same model, alternating in blocks, each over STEPS steps; device events time
the whole step (replay + optimizer) and the optimizer launch alone.  Kernel times: run this under rocprofv3 --kernel-trace --stats.

    python tools/micro/ema_cost.py [STEPS=200] [BLOCK=20]"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import torch.nn as nn  # noqa: E402

import sbgm_danra_amd as S  # noqa: E402
from sbgm_danra_amd.ema import ModelEMA  # noqa: E402

STEPS = int(sys.argv[1]) if len(sys.argv) > 1 else 200
BLOCK = int(sys.argv[2]) if len(sys.argv) > 2 else 20


def main():
    dev = torch.device("cuda")
    torch.manual_seed(0)
    enc = S.Encoder(4, 256, block_layers=[2, 2, 2, 2], n_heads=4)          # 4 condition channels, as bench.py builds C3
    dec = S.Decoder(512, 1, 256, n_heads=4, norm="group", gn_groups=8, activation=nn.SiLU)
    net = S.ScoreNet(S.marginal_prob_std_fn, enc, dec, device=dev, debug_pre_sigma_div=False)
    net.train()
    print(f"parameters: {sum(p.numel() for p in net.parameters()) / 1e6:.2f} M", flush=True)
    opt = S.optim.Adam(net.parameters(), lr=5e-4, weight_decay=1e-6)
    ema = ModelEMA(net, 0.9999)
    ema.reset()
    g = torch.Generator().manual_seed(42)
    x, cond = torch.randn(8, 1, 128, 128, generator=g).to(dev), torch.randn(8, 4, 128, 128, generator=g).to(dev)

    def fwd_bwd():
        loss = S.loss_fn(net, x, S.marginal_prob_std_fn, cond_img=cond)
        loss.backward()
        return loss
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            opt.zero_grad(set_to_none=True)
            fwd_bwd()
            opt.step()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    opt.zero_grad(set_to_none=True)
    with torch.cuda.graph(graph):
        fwd_bwd()

    def run(on, n):
        opt.ema = ema if on else None
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
              for _ in range(n)]
        for a, b, c in ev:
            a.record()
            graph.replay()
            b.record()
            opt.step()
            c.record()
        torch.cuda.synchronize()
        return [a.elapsed_time(c) for a, b, c in ev], [b.elapsed_time(c) for a, b, c in ev]
    for on in (False, True, False, True):                       # warm-up of both variants (descriptor tables, clocks)
        run(on, BLOCK)
    res = {False: ([], []), True: ([], [])}
    done = 0
    while done < STEPS:
        for on in (False, True):
            s, o = run(on, BLOCK)
            res[on][0].extend(s)
            res[on][1].extend(o)
        done += BLOCK
    med = lambda v: sorted(v)[len(v) // 2]                      # noqa: E731
    mean = lambda v: sum(v) / len(v)                            # noqa: E731
    for on in (False, True):
        s, o = res[on]
        print(f"ema={'on ' if on else 'off'}: step median {med(s) * 1e3:8.1f} us  mean {mean(s) * 1e3:8.1f} us | "
              f"optimizer median {med(o) * 1e3:7.1f} us  mean {mean(o) * 1e3:7.1f} us  ({len(s)} steps)", flush=True)
    d_step = med(res[True][0]) - med(res[False][0])
    d_opt = med(res[True][1]) - med(res[False][1])
    print(f"EMA cost: step median +{d_step * 1e3:.1f} us, optimizer median +{d_opt * 1e3:.1f} us; updates {ema.num_updates}", flush=True)
    assert all(torch.isfinite(p).all() for p in ema.shadow.parameters())


if __name__ == "__main__":
    main()
