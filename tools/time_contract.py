"""Timings of the contraction engine (tnco_amd/contraction.py, csrc/contract.hip) on one GPU, against torch.tensordot
on the same GPU along the same path.

    python tools/time_contract.py [--out profiles/contract_timing.txt]

Legs: one large square step per dtype (TFLOP/s: 2 flops per real MAC, 8 per complex MAC); one skinny step (effective
GB/s: operands read once + result written once, against the ~6.3 TB/s an MI355X streams); a sliced Sycamore-53
amplitude from the finite-width optimizer (wall time, device time, launches per slice, MACs/s).  Engine figures are its
own device time (events around the slice loop: the copies in and out are excluded, as they are for torch, whose
operands stay on the device).
"""
from __future__ import annotations

import argparse
import math
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

import torch  # noqa: E402  (torch's HIP runtime first: tnco_amd/_lib.py)

from tnco_amd import contraction as ctr  # noqa: E402
from tnco_amd import synthetic as syn  # noqa: E402
from tnco_amd.app import tn as tnmod  # noqa: E402
from tnco_amd.app.app import Optimizer  # noqa: E402

FLOPS_PER_MAC = {np.float32: 2, np.float64: 2, np.complex64: 8, np.complex128: 8}
TORCH = {np.float32: torch.float32, np.float64: torch.float64, np.complex64: torch.complex64,
         np.complex128: torch.complex128}


def _rand(shape, dtype, rng):
    a = rng.standard_normal(shape)
    if np.dtype(dtype).kind == "c":
        a = a + 1j * rng.standard_normal(shape)
    return (a / math.sqrt(shape[-1])).astype(dtype)


def _torch_time(fn, reps=5):
    fn()
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    for _ in range(reps):
        fn()
    ev[1].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1]) / 1e3 / reps


def _engine_time(call, reps=3):
    call()
    return min(call().device_s for _ in range(reps))


def square(lines, n):
    lines.append(f"## large square step: Z[i,j] = sum_k X[i,k] Y[k,j], M = N = K = {n} (tiled LDS kernel)")
    lines.append(f"{'dtype':>10} {'engine s':>10} {'engine TFLOP/s':>15} {'torch s':>10} {'torch TFLOP/s':>14} {'ratio':>6}")
    rng = np.random.RandomState(0)
    for dt in (np.float32, np.float64, np.complex64, np.complex128):
        x, y = _rand((n, n), dt, rng), _rand((n, n), dt, rng)
        t_e = _engine_time(lambda: ctr.contract([(0, 1)], [("i", "k"), ("k", "j")], [x, y]))
        tx, ty = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
        t_t = _torch_time(lambda: torch.tensordot(tx, ty, dims=([1], [0])))
        fl = FLOPS_PER_MAC[dt] * n ** 3
        lines.append(f"{np.dtype(dt).name:>10} {t_e:10.4f} {fl / t_e / 1e12:15.2f} {t_t:10.4f} {fl / t_t / 1e12:14.2f} "
                     f"{t_t / t_e:6.2f}")
        del tx, ty
    print("\n".join(lines[-5:]), flush=True)


def skinny(lines):
    lines.append("")
    lines.append("## skinny steps (streaming / split-K kernels): effective GB/s = (operands + result bytes) / time")
    lines.append(f"{'step':>40} {'engine s':>10} {'engine GB/s':>12} {'torch s':>10} {'torch GB/s':>11} {'ratio':>6}")
    rng = np.random.RandomState(1)
    cases = [("X[i,k] Y[k,j], i=2^24 k=8 j=4 f32", (1 << 24, 8), (8, 4), np.float32),
             ("X[i,k] Y[k], i=2^22 k=16 f32 (matrix-vector)", (1 << 22, 16), (16,), np.float32),
             ("X[i] Y[j] outer, i=2^14 j=2^12 f32", (1 << 14,), (1 << 12,), np.float32),
             ("X[i,k] Y[k], i=4 k=2^24 f64 (long sum)", (4, 1 << 24), (1 << 24,), np.float64)]
    for name, sx, sy, dt in cases:
        x, y = _rand(sx, dt, rng), _rand(sy, dt, rng)
        ix = ("i", "k")[:len(sx)]
        iy = ("k", "j")[:len(sy)] if len(sx) == 2 else ("j",)
        res = ctr.contract([(0, 1)], [ix, iy], [x, y])
        t_e = _engine_time(lambda: ctr.contract([(0, 1)], [ix, iy], [x, y]))
        tx, ty = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
        dims = ([1], [0]) if len(sx) == 2 else 0
        t_t = _torch_time(lambda: torch.tensordot(tx, ty, dims=dims))
        nbytes = (x.nbytes + y.nbytes + res.array.nbytes)
        lines.append(f"{name:>40} {t_e:10.5f} {nbytes / t_e / 1e9:12.1f} {t_t:10.5f} {nbytes / t_t / 1e9:11.1f} "
                     f"{t_t / t_e:6.2f}")
        del tx, ty
    print("\n".join(lines[-6:]), flush=True)


def sycamore(lines, depth, max_width, max_slices):
    lines.append("")
    ts, d, o = syn.sycamore53_tn(depth=depth)
    tn0 = tnmod.TensorNetwork([tnmod.Tensor(xs, [d] * len(xs)) for xs in ts], output_inds=o)
    t0 = time.perf_counter()
    tn, res = Optimizer(method="sa", max_width=max_width, seed=0).optimize(tn0, betas=(0, 50), n_steps=200,
                                                                          n_runs=256)
    t_opt = time.perf_counter() - t0
    r0 = res[0]
    rng = np.random.RandomState(2)
    arrays = [(_rand(tuple(d for _ in xs), np.complex64, rng) * 1.0).astype(np.complex64) for xs in ts]
    fused = ctr.contract(tn.tags["fuse_path"], tn0.ts_inds, arrays, tn0.output_inds)
    leaves = fused.array if isinstance(fused.array, list) else [fused.array]
    p = ctr.plan(r0.path, tn.ts_inds, [a.shape for a in leaves], tn.output_inds, slices=r0.slices)
    n = min(p.n_slices, max_slices)
    t0 = time.perf_counter()
    r = ctr.contract(r0.path, tn.ts_inds, leaves, tn.output_inds, slices=r0.slices, slice_range=(0, n))
    wall = time.perf_counter() - t0
    steps = len(r0.path)
    lines.append(f"## sliced Sycamore-53 amplitude, depth {depth}, complex64: {len(ts)} tensors, fused to {len(tn.ts_inds)}; "
                 f"finite-width SA (max_width {max_width}, 256 runs x 200 sweeps, {t_opt:.1f} s): cost {r0.cost}, "
                 f"{len(r0.slices)} sliced indices, {p.n_slices} assignments")
    lines.append(f"  run of assignments [0, {n}): wall {wall:.3f} s (copies in/out included), device {r.device_s:.3f} s; "
                 f"{steps} steps, {r.launches} launches = {r.launches / n:.1f} per slice, "
                 f"{r.device_s / n * 1e6:.1f} us per slice ({r.device_s / max(r.launches, 1) * 1e6:.2f} us per launch)")
    lines.append(f"  MACs {r.macs} (= cost x {n}/{p.n_slices}: {r.macs * p.n_slices == p.macs_per_slice * p.n_slices * n}), "
                 f"{r.macs / r.device_s / 1e9:.2f} GMAC/s on the device, peak device bytes {r.peak_device_bytes}")
    big = max(op["H"] * op["M"] * op["N"] * op["K"] for op in p.ops)
    lines.append(f"  largest step of a slice: {big} MACs; launches/slice x ~launch time bounds the rate: the steps of a "
                 "slice are small (width <= max_width), so a slice is launch-bound")
    print("\n".join(lines[-4:]), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "contract_timing.txt"))
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--depth", type=int, default=8)
    ap.add_argument("--max-width", type=float, default=14)
    ap.add_argument("--max-slices", type=int, default=4096)
    a = ap.parse_args()
    lines = [f"# tools/time_contract.py on {torch.cuda.get_device_name(0)}; torch {torch.__version__}", ""]
    square(lines, a.n)
    skinny(lines)
    sycamore(lines, a.depth, a.max_width, a.max_slices)
    Path(a.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
