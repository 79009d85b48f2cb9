"""What a training step costs between the backward pass and the next forward pass, at base.json's parameter count (12.2 M): the path of the commit before the fused
optimiser against nrs_optimizer_step, in one process, timed alternately with stream events after `--warmup` untimed rounds (median and 10th..90th percentile of
`--reps`).  A first measurement, no bar.

  (a) before: the backward pass's memset of the gradient (hipMemsetAsync, 49 MB) + params.grad.add_(grad, alpha=1/loss_scale) + torch.optim.Adam.step()
      + params.to(float16) + nrs_model_set_params_device (a 24 MB device-to-device copy and the fragment kernel).
  (b) nrs_optimizer_step with zero_grad on an optimiser bound to the model, the fragment kernel included: four variants (NRS_OPTIMIZER_VARIANT, read when an optimiser
      is created): the EMA in the step's launch or in one of its own, the bias table staged in LDS or read through L2.  The first of the four is what the library does.
Both against two gradients: a real one (nrs_network_backward over 2^18 random samples: 7 % of the elements are exactly zero and skipped) and one without a
zero (the worst case).  (b)'s gradient is refilled before every timed call (the step clears it), outside the timed span.
For (b): the bytes the rule must move -- 42 B per live element (4 grad + 16 state read, 16 state + 2 fp16 + 4 grad written) + 8 B of EMA, 4 B + 10 B of EMA (it reads
the stored fp16) per skipped one -- over the time.  --json adds one machine-readable line.  Needs a GPU.

    python tools/optimizer_probe.py [--reps 15] [--warmup 3] [--log2-hashmap 19] [--json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
VARIANTS = ((0, "EMA fused, table in LDS"), (1, "EMA in its own launch, table in LDS"), (2, "EMA fused, table in L2"), (3, "EMA in its own launch, table in L2"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--log2-hashmap", type=int, default=19)
    ap.add_argument("--json", action="store_true")
    args = ap.parse_args()
    import torch
    from nerfshop_amd import runtime as rt, synth
    from nerfshop_amd.torch_module import LOSS_SCALE, N_MLP_PARAMS, initial_params

    dev = "cuda:0"
    ctx = rt.Context(0)
    desc = synth.model_desc(1, log2_hashmap_size=args.log2_hashmap)
    init = initial_params(int(rt.NerfNetwork(ctx, desc, cell_cache_bytes=0).n_params()), 7)
    init[N_MLP_PARAMS:] *= 5e3  # grid entries U(-0.5, 0.5): features of the size a trained snapshot has
    n = init.numel()

    # the two gradients
    net_a = rt.NerfNetwork(ctx, desc, cell_cache_bytes=0)
    net_a.set_params_device(init.to(torch.float16).to(dev))
    gen = torch.Generator(device=dev).manual_seed(3)
    ns = 1 << 18
    coords = torch.rand((ns, 7), generator=gen, device=dev) * 0.96 + 0.02
    dl = torch.zeros((ns, 16), dtype=torch.float16, device=dev)
    dl[:, :4] = torch.randn((ns, 4), generator=gen, device=dev).to(torch.float16)
    real = torch.empty(n, dtype=torch.float32, device=dev)
    net_a.backward(None, coords, dl, real, None, accumulate=False)
    dense = torch.randn(n, generator=gen, device=dev) * 1e-2 + 1e-6
    dense[dense == 0] = 1e-6
    grads = {"real (2^18 samples)": real, "no zero anywhere": dense}

    # (a)
    params = torch.nn.Parameter(init.to(dev))
    params.grad = torch.zeros_like(params)
    adam = torch.optim.Adam([params], lr=1e-2, betas=(0.9, 0.99), eps=1e-15)
    scratch = torch.empty(n, dtype=torch.float32, device=dev)

    def path_a(g):
        scratch.zero_()                                     # nrs_network_backward(accumulate = 0): hipMemsetAsync of the gradient
        params.grad.add_(g, alpha=1.0 / LOSS_SCALE)
        adam.step()
        net_a.set_params_device(params.detach().to(torch.float16))

    # (b)
    opts = {}
    for variant, name in VARIANTS:
        os.environ["NRS_OPTIMIZER_VARIANT"] = str(variant)
        net = rt.NerfNetwork(ctx, desc, cell_cache_bytes=0)
        opt = rt.Optimizer(ctx, network=net)
        opt.set_weights(init.to(dev))
        opts[name] = (net, opt)
    os.environ.pop("NRS_OPTIMIZER_VARIANT")
    gbuf = torch.empty(n, dtype=torch.float32, device=dev)

    def timed(fn, before=None):
        if before is not None:
            before()
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        e.synchronize()
        return s.elapsed_time(e)

    rows, result = [], {"n_params": n}
    for gname, g in grads.items():
        live = int(((g != 0) | (torch.arange(n, device=dev) < N_MLP_PARAMS)).sum())
        must_move = live * 50 + (n - live) * 14
        times = {"(a) before": []}
        times.update({f"(b) {name}": [] for _, name in VARIANTS})
        for rep in range(args.warmup + args.reps):
            t = {"(a) before": timed(lambda: path_a(g))}
            for _, name in VARIANTS:
                opt = opts[name][1]
                t[f"(b) {name}"] = timed(lambda: opt.step(gbuf, loss_scale=LOSS_SCALE, lr=1e-2, zero_grad=True), before=lambda: gbuf.copy_(g))
            if rep >= args.warmup:
                for k, v in t.items():
                    times[k].append(v)
        assert float(gbuf.abs().max()) == 0
        for k, v in times.items():
            med, lo, hi = np.median(v), np.percentile(v, 10), np.percentile(v, 90)
            rate = f"{must_move / (med * 1e-3) / 1e12:.2f} TB/s of {must_move / 1e6:.0f} MB" if k.startswith("(b)") else ""
            rows.append((gname, f"{live / n:.3f}", k, f"{med:.3f}", f"{lo:.3f}..{hi:.3f}", rate))
            result[f"{gname} | {k}"] = {"median_ms": float(med), "p10_ms": float(lo), "p90_ms": float(hi), "live_share": live / n, "must_move_bytes": must_move}
    print(f"{ctx.device_name}; {n} parameters; {args.reps} timed rounds after {args.warmup}")
    print("| gradient | live share | path | median ms | p10..p90 ms | achieved |")
    print("|---|---|---|---|---|---|")
    for r in rows:
        print("| " + " | ".join(r) + " |")
    if args.json:
        print(json.dumps(result))


if __name__ == "__main__":
    main()
