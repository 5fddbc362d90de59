"""Speed probe of the verification kernels (csrc/verify.hip) at the full DANRA domain, 589 x 789, with N = 64 generated
samples against one truth per sample and an ensemble of M = 64 members.  One JSON line: milliseconds per call (median of
--reps timed calls after a warm-up) and effective GB/s = the bytes each call must move at least (inputs read once, outputs
written once) / time.  The spectrum figure times the binning kernel alone on precomputed |F|^2 (the FFT is torch's).

Usage: python tools/eval_speed.py [--reps 20]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from sbgm_danra_amd import _native as N  # noqa: E402
from sbgm_danra_amd import verification as V  # noqa: E402

H, W, NS, M = 589, 789, 64, 64


def time_ms(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return sorted(ts)[len(ts) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    reps = ap.parse_args().reps
    dev = torch.device("cuda")
    g = torch.Generator(device=dev).manual_seed(0)
    HW = H * W
    gen = torch.randn(NS, H, W, device=dev, generator=g)
    obs = torch.randn(NS, H, W, device=dev, generator=g)
    ens = torch.randn(M, H, W, device=dev, generator=g)
    mask = (torch.rand(H, W, device=dev, generator=g) < 0.6).to(torch.uint8)
    x = gen - gen.mean(dim=(1, 2), keepdim=True)
    power = torch.fft.fft2(x).abs().square().float().contiguous()
    ok = torch.ones(NS, dtype=torch.uint8, device=dev)
    nb = max(H, W) // 2 + 1
    psd = torch.empty(nb, dtype=torch.float64, device=dev)
    cnt = torch.empty(nb, dtype=torch.int64, device=dev)
    nf = torch.empty(1, dtype=torch.int64, device=dev)
    ws = torch.empty(N.lib().sbgm_radial_spectrum_workspace_bytes(H, W), dtype=torch.uint8, device=dev)

    def spectrum():
        N.check(N.lib().sbgm_radial_spectrum(power.data_ptr(), ok.data_ptr(), NS, H, W, psd.data_ptr(), cnt.data_ptr(), nf.data_ptr(),
                                             ws.data_ptr(), N.stream()))

    cases = {
        "error_stats": (lambda: V.error_stats(gen, obs, mask), 2 * NS * HW * 4 + HW + HW * 16),
        "histogram_150": (lambda: V.histogram(gen, 150, -4.0, 4.0, ref=obs, mask=mask), 2 * NS * HW * 4 + HW),
        "ensemble_scores": (lambda: V.ensemble_scores(ens, obs[0], mask, seed=1), M * HW * 4 + HW * 5 + HW * 16),
        "radial_spectrum": (spectrum, NS * HW * 4),
        "rapsd_with_fft": (lambda: V.rapsd(gen), NS * HW * 4),
    }
    out = {"shape": [H, W], "N": NS, "M": M, "device": torch.cuda.get_device_name(0)}
    for name, (fn, nbytes) in cases.items():
        ms = time_ms(fn, reps)
        out[name] = {"ms": round(ms, 4), "GBps": round(nbytes / ms / 1e6, 1)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
