#!/usr/bin/env python3
"""A/B of the context encoder with its BatchNorm in training mode: the channels-last route with the BatchNorm kernels of
csrc/norm_bn.hip (extractor.TRAIN_BN = True, the default) against the framework's NCHW modules on MIOpen (TRAIN_BN = False, what
ran before), with the frozen route (eval-mode statistics, freeze_bn) as a third column.  Forward + backward of
BasicEncoder(output_dim=256, norm_fn='batch') at 1 x 3 x 368 x 768 and 1 x 3 x 432 x 1024 (the flow-supervisor recipe's crop and
frame) and 8 x 3 x 368 x 496 (a chairs batch), and one SemiTrainStep on GMAL2L at the recipe size (crop 368 x 768 in a 432 x 1024
frame, 12 + 12 iterations) with the model's BatchNorm in training mode, switch on / off.

    python scripts/train_bn_ab.py [--out profiles/train_bn_ab.txt] [--runs 20] [--step-runs 6]

One process, eager launches.  Every call is timed between device events; every path is warmed up at the shape it is timed at;
the paths alternate inside every round, so that all see the same neighbours on the machine; reported are the median and the range.
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = ((1, 368, 768), (1, 432, 1024), (8, 368, 496))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "train_bn_ab.txt"))
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--step-runs", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    import torch
    import flow_supervisor_amd.core.extractor as X
    from flow_supervisor_amd.core.gma_l2l import GMAL2L
    from flow_supervisor_amd.train import SemiTrainStep
    if not torch.cuda.is_available():
        sys.exit("train_bn_ab: no GPU visible; nothing is measured without one")
    dev = "cuda"
    torch.manual_seed(0)

    def events(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    def alternate(paths, runs):
        """paths: [(name, fn)] -> {name: [ms]}; a.warmup calls each, then `runs` rounds of one call each."""
        for _, fn in paths:
            for _ in range(a.warmup):
                fn()
        torch.cuda.synchronize()
        ms = {name: [] for name, _ in paths}
        for _ in range(runs):
            for name, fn in paths:
                ms[name].append(events(fn))
        return ms

    def fmt(v):
        return f"{statistics.median(v):>10.3f}{min(v):>9.3f}{max(v):>9.3f}"

    lines = ["Context encoder with BatchNorm in training mode, MI355X, one process, eager launches; ms between device events, median (min .. max).",
             f"{a.warmup} warm-up calls of every path at its shape, then rounds that run every path once (alternating).", "",
             f"forward + backward of BasicEncoder(output_dim=256, norm_fn='batch'), {a.runs} rounds",
             f"{'input':<20}{'path':<50}{'ms median':>10}{'min':>9}{'max':>9}"]
    verdicts = []
    for B, H, W in SHAPES:
        enc = X.BasicEncoder(output_dim=256, norm_fn="batch").to(dev)
        x = torch.randn(B, 3, H, W, device=dev)

        def fwd_bwd(train, switch):
            def fn():
                X.TRAIN_BN = switch
                enc.train(train)
                enc.zero_grad(set_to_none=True)
                enc(x).square().mean().backward()
                X.TRAIN_BN = True
            return fn

        paths = [("training mode, BatchNorm kernels (TRAIN_BN on)", fwd_bwd(True, True)),
                 ("training mode, framework modules (TRAIN_BN off)", fwd_bwd(True, False)),
                 ("frozen (eval-mode statistics)", fwd_bwd(False, True))]
        ms = alternate(paths, a.runs)
        for name, _ in paths:
            lines.append(f"{f'{B} x 3 x {H} x {W}':<20}{name:<50}{fmt(ms[name])}")
        on, off, frozen = (statistics.median(ms[name]) for name, _ in paths)
        verdicts.append(f"{B} x 3 x {H} x {W}: kernels {on:.2f} ms, framework {off:.2f} ms ({off / on:.2f}x), frozen {frozen:.2f} ms: the kernels' "
                        f"route is {'FASTER than' if on < off else 'SLOWER than'} the framework's and "
                        f"{'slower than' if on > frozen else 'not slower than'} the frozen one")
        del enc

    model = GMAL2L(argparse.Namespace(mixed_precision=False, num_heads=1, position_only=False, position_and_content=False)).to(dev).train()
    with torch.no_grad():
        model.update_block.aggregator.gamma.fill_(0.1)
    g = torch.Generator(device=dev).manual_seed(1234)
    FH, FW, ch, cw = 432, 1024, 368, 768

    def pair():
        i1 = torch.rand(1, 3, FH, FW, device=dev, generator=g) * 255.0
        i2 = (torch.roll(i1, shifts=(3, -5), dims=(2, 3)) + 2.0 * torch.randn(1, 3, FH, FW, device=dev, generator=g)).clamp(0, 255)
        return i1, i2

    def sample(frame, oy, ox):
        f1, f2 = frame
        c1, c2 = (f[:, :, oy:oy + ch, ox:ox + cw].contiguous() for f in (f1, f2))
        return (c1, c2, f1, f2, ox, oy, torch.randn(1, 2, ch, cw, device=dev, generator=g) * 4.0,
                (torch.rand(1, ch, cw, device=dev, generator=g) > 0.1).float())

    sup, unsup = sample(pair(), 40, 136), sample(pair(), 16, 200)
    step = SemiTrainStep(model, lr=1e-6, wdecay=0.0, iters=12, gamma=0.85, unsup_lambda=0.25)      # train_semi.sh:3-11
    assert step._bn_training()

    def semi(switch):
        def fn():
            X.TRAIN_BN = switch
            step(sup, unsup)
            X.TRAIN_BN = True
        return fn

    paths = [("BatchNorm kernels (TRAIN_BN on)", semi(True)), ("framework modules (TRAIN_BN off)", semi(False))]
    ms = alternate(paths, a.step_runs)
    lines += ["", f"SemiTrainStep on GMAL2L, BatchNorm in training mode (the sequential two-pass step), crop {ch} x {cw} in {FH} x {FW}, 12 + 12 "
              f"iterations, {a.step_runs} rounds", f"{'':<20}{'path':<50}{'ms median':>10}{'min':>9}{'max':>9}"]
    for name, _ in paths:
        lines.append(f"{'':<20}{name:<50}{fmt(ms[name])}")
    on, off = (statistics.median(ms[name]) for name, _ in paths)
    verdicts.append(f"SemiTrainStep GMAL2L: kernels {on:.1f} ms, framework {off:.1f} ms per step ({off / on:.3f}x)")
    lines += [""] + verdicts
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
