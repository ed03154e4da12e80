"""Timings of the contraction engine (tnco_amd/contraction.py, csrc/contract.hip) on one GPU, against torch.tensordot
on the same GPU along the same path.

    python tools/time_contract.py [--out profiles/contract_timing.txt]

Legs: one large square step per dtype (TFLOP/s: 2 flops per real MAC, 8 per complex MAC); one skinny step (effective
GB/s: operands read once + result written once, against the ~6.3 TB/s an MI355X streams); a sliced Sycamore-53
amplitude from the finite-width optimizer (wall time, device time, launches per slice, MACs/s); P output bitstrings
of that circuit in one projected call (`--projs`: the 53 output indices sparse, an infinite-memory path from
optimize(n_projs=P)) against a loop of plain contract() calls over leaves indexed at one bitstring each, along the same
path; the storage mode (`--storage`: the large square step in float32 and complex64 with `storage` unset, float16 and
bfloat16, and the sliced Sycamore leg once more with storage="bfloat16"); slice batches (`--slice-batch`: the sliced
Sycamore leg with slice_batch None, 1, 8 and 64, plain, in storage mode and with scaling); the compute mode
(`--compute`: the large square step in float32 and complex64 with compute=None, compute="bf16x3" and
storage="bfloat16" in one process, and the sliced Sycamore leg with compute=None and "bf16x3"); the path kernel
(`--path-kernel`: the sliced Sycamore leg with path_kernel=None, slice_batch=64 and path_kernel 64, 256 and 1024 in one
process); hoisting (`--hoist`: the sliced Sycamore leg with hoist=None and hoist=True, unbatched and with
slice_batch=64, in one process); the matrix mode (`--matrix`: the large square step in the four dtypes with compute=None
and compute="matrix", in float32 and complex64 also with compute="bf16x3" and storage="bfloat16", and torch, in one
process); operands read in place (`--indirect`: the sliced Sycamore leg with slice_batch None and 64, hoist None and True,
each with indirect=None and indirect=True, and one bandwidth-bound step whose 2^26-element operand lies in reversed axis
order, in one process); reuse (`--reuse`: the sliced Sycamore leg, unbatched, with hoist=None, hoist=True, reuse=True,
reuse=True with slice_order="reuse", and that with indirect=True, and the same five on a deeper network whose assignments
take milliseconds, every ratio against hoist=True, in one process); the wide accumulation (`--accumulate`: the sliced
Sycamore leg with accumulate=None and "float64", unbatched, with slice_batch=64 and hoist=True, and with path_kernel=1024,
and the error of each against the same plan in complex128, in one process); the resident use (`--resident`: wall time
per call of contract() and of one Contractor run with numpy arrays, with every leaf bound from numpy, and with every leaf
bound from torch tensors and the result written into a tensor, on the sliced Sycamore leg under path_kernel=1024 and on
the bandwidth-bound step of the indirect leg, in one process); leaf sets (`--many`: Contractor.run_many against the loop of
Contractor.run() over the same sets on the same Contractor, wall time per set, on the sliced Sycamore leg under
path_kernel=1024: 1024 sets of one assignment each, and 8 sets of every assignment, in one process); sampling (`--sample`:
one gate-by-gate walk of a random circuit of 1-qubit gates and CZs for all samples at once, through sampling.Sampler --
walkers on the device, indexed leaves, the choice in a kernel -- and through the loop that run_many allows without them,
on the same Contractors, in one process).  Engine figures are its
own device time (events around the slice loop: the copies in and out are excluded, as they are for torch, whose
operands stay on the device); the resident leg measures what that leaves out.
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


def storage(lines, n, depth, max_width, max_slices):
    """The storage mode against the plain engine on the same box: the large square step (the MFMA kernel against the
    tiled LDS kernel), and the sliced Sycamore amplitude with bfloat16 leaves and intermediates."""
    lines.append("")
    lines.append(f"## storage mode, large square step M = N = K = {n}: leaves in float16 / bfloat16, float32 sums on the "
                 "matrix cores (ct_mfma_tiled_kernel) against the tiled LDS kernel (storage unset)")
    lines.append(f"{'dtype':>10} {'storage':>9} {'engine s':>10} {'TFLOP/s':>9} {'unset / this':>13} {'rel. diff to unset':>19}")
    rng = np.random.RandomState(4)
    for dt in (np.float32, np.complex64):
        x, y = _rand((n, n), dt, rng), _rand((n, n), dt, rng)
        fl = FLOPS_PER_MAC[dt] * n ** 3
        base = t_base = None
        for st in (None, "float16", "bfloat16"):
            call = lambda st=st: ctr.contract([(0, 1)], [("i", "k"), ("k", "j")], [x, y], storage=st)  # noqa: E731
            r = call()
            t = min(r.device_s, _engine_time(call))
            if st is None:
                base, t_base = r.array, t
            diff = float(np.linalg.norm(r.array - base) / np.linalg.norm(base))
            lines.append(f"{np.dtype(dt).name:>10} {str(st):>9} {t:10.5f} {fl / t / 1e12:9.1f} {t_base / t:13.2f} {diff:19.2e}")
            del r
        del base, x, y
    ts, d, o = syn.sycamore53_tn(depth=depth)
    tn0 = tnmod.TensorNetwork([tnmod.Tensor(xs, [d] * len(xs)) for xs in ts], output_inds=o)
    tn, res = Optimizer(method="sa", max_width=max_width, seed=0).optimize(tn0, betas=(0, 50), n_steps=200, n_runs=256)
    r0 = res[0]
    rng = np.random.RandomState(2)
    # unit-modulus entries give an amplitude of about 2^(indices / 2), far beyond float32 here (the sycamore leg above
    # times such a run; its numbers are not finite): every tensor is scaled so that the amplitude stays near 1
    n_inds = len({x for xs in ts for x in xs})
    scale = 2.0 ** (-n_inds / (2 * len(ts)))
    arrays = [(_rand(tuple(d for _ in xs), np.complex64, rng) * scale).astype(np.complex64) for xs in ts]
    fused = ctr.contract(tn.tags["fuse_path"], tn0.ts_inds, arrays, tn0.output_inds)
    leaves = fused.array if isinstance(fused.array, list) else [fused.array]
    p = ctr.plan(r0.path, tn.ts_inds, [a.shape for a in leaves], tn.output_inds, slices=r0.slices)
    m = min(p.n_slices, max_slices)
    runs = {st: ctr.contract(r0.path, tn.ts_inds, leaves, tn.output_inds, slices=r0.slices, slice_range=(0, m), storage=st)
            for st in (None, "bfloat16")}
    a, b = runs[None], runs["bfloat16"]
    err = float(np.linalg.norm(np.ravel(b.array - a.array)) / np.linalg.norm(np.ravel(a.array)))
    lines.append(f"## storage mode, sliced Sycamore-53 amplitude, depth {depth}, complex64, max_width {max_width}, "
                 f"assignments [0, {m}): storage unset: device {a.device_s:.3f} s, peak device bytes {a.peak_device_bytes}; "
                 f"storage=\"bfloat16\": device {b.device_s:.3f} s, peak device bytes {b.peak_device_bytes}, relative "
                 f"error to the complex64 run {err:.2e}; launches {dict(zip(ctr.KERNEL_PATHS, b.kernel_launches))}")
    print("\n".join(lines[-9:]), flush=True)


def scaling(lines, n, depth, max_width, max_slices):
    """What per-tensor scaling costs in time, storage mode with and without it on the same box in the same run: a large
    step whose result is stored (staging + narrowing pass) followed by a product with a few vectors, and the sliced
    Sycamore amplitude of the storage leg."""
    lines.append("")
    lines.append(f"## scaling=\"tensor\" against storage mode alone, A ({n}, {n}) B ({n}, {n}) -> Z stored, Z w ({n}, 8): "
                 "the MFMA step writes float32 staging, ct_scale_narrow_kernel rounds it to storage")
    lines.append(f"{'dtype':>10} {'storage':>9} {'scaling':>8} {'engine s':>10} {'scaled / unscaled':>18} {'launches':>9} {'narrow':>7}")
    rng = np.random.RandomState(5)
    ts = [("i", "k"), ("k", "j"), ("j", "l")]
    for dt in (np.float32, np.complex64):
        arrays = [(_rand(shape, dt, rng) * np.float32(n ** -0.5)).astype(dt) for shape in ((n, n), (n, n), (n, 8))]
        for st in ("float16", "bfloat16"):
            t_plain = None
            for sc in (None, "tensor"):
                call = lambda st=st, sc=sc: ctr.contract([(0, 1), (0, 1)], ts, arrays, storage=st, scaling=sc)  # noqa: E731
                r = call()
                t = min(r.device_s, _engine_time(call))
                t_plain = t if sc is None else t_plain
                lines.append(f"{np.dtype(dt).name:>10} {st:>9} {str(sc):>8} {t:10.5f} {t / t_plain:18.3f} {r.launches:9d} "
                             f"{r.narrow_launches:7d}")
                del r
        del arrays
    ts, d, o = syn.sycamore53_tn(depth=depth)
    tn0 = tnmod.TensorNetwork([tnmod.Tensor(xs, [d] * len(xs)) for xs in ts], output_inds=o)
    tn, res = Optimizer(method="sa", max_width=max_width, seed=0).optimize(tn0, betas=(0, 50), n_steps=200, n_runs=256)
    r0 = res[0]
    rng = np.random.RandomState(2)
    n_inds = len({x for xs in ts for x in xs})
    scale = 2.0 ** (-n_inds / (2 * len(ts)))  # (as in the storage leg: the amplitude stays near 1)
    arrays = [(_rand(tuple(d for _ in xs), np.complex64, rng) * scale).astype(np.complex64) for xs in ts]
    fused = ctr.contract(tn.tags["fuse_path"], tn0.ts_inds, arrays, tn0.output_inds)
    leaves = fused.array if isinstance(fused.array, list) else [fused.array]
    p = ctr.plan(r0.path, tn.ts_inds, [a.shape for a in leaves], tn.output_inds, slices=r0.slices)
    m = min(p.n_slices, max_slices)
    run = lambda st, sc: ctr.contract(r0.path, tn.ts_inds, leaves, tn.output_inds, slices=r0.slices,  # noqa: E731
                                      slice_range=(0, m), storage=st, scaling=sc)
    base = run(None, None)
    lines.append(f"## scaling, sliced Sycamore-53 amplitude, depth {depth}, complex64, max_width {max_width}, assignments "
                 f"[0, {m}); storage unset: device {base.device_s:.3f} s, {base.launches} launches")
    for st in ("float16", "bfloat16"):
        for sc in (None, "tensor"):
            r = run(st, sc)
            err = float(np.linalg.norm(np.ravel(r.array - base.array)) / np.linalg.norm(np.ravel(base.array)))
            lines.append(f"  storage={st} scaling={sc}: device {r.device_s:.3f} s, {r.launches} launches of which "
                         f"{r.narrow_launches} narrowing passes, peak device bytes {r.peak_device_bytes}, relative error to "
                         f"the complex64 run {err:.2e}")
    print("\n".join(lines[-16:]), flush=True)


def slice_batch(lines, depth, max_width, max_slices, batches=(None, 1, 8, 64)):
    """Slice assignments per launch on the sliced Sycamore amplitude of the storage leg: device time (the minimum and
    the spread of three runs after a warm-up, all in this process), launches, memory and rate per batch size, plain, in
    storage mode and with scaling; every batched result is compared bit for bit with the unbatched one of its mode."""
    lines.append("")
    ts, d, o = syn.sycamore53_tn(depth=depth)
    tn0 = tnmod.TensorNetwork([tnmod.Tensor(xs, [d] * len(xs)) for xs in ts], output_inds=o)
    tn, res = Optimizer(method="sa", max_width=max_width, seed=0).optimize(tn0, betas=(0, 50), n_steps=200, n_runs=256)
    r0 = res[0]
    rng = np.random.RandomState(2)
    n_inds = len({x for xs in ts for x in xs})
    scale = 2.0 ** (-n_inds / (2 * len(ts)))  # (as in the storage leg: the amplitude stays near 1)
    arrays = [(_rand(tuple(d for _ in xs), np.complex64, rng) * scale).astype(np.complex64) for xs in ts]
    fused = ctr.contract(tn.tags["fuse_path"], tn0.ts_inds, arrays, tn0.output_inds)
    leaves = fused.array if isinstance(fused.array, list) else [fused.array]
    p = ctr.plan(r0.path, tn.ts_inds, [a.shape for a in leaves], tn.output_inds, slices=r0.slices)
    m = min(p.n_slices, max_slices)
    lines.append(f"## slice_batch, sliced Sycamore-53 amplitude, depth {depth}, complex64, max_width {max_width}, cost "
                 f"{r0.cost}, {len(r0.path)} steps, assignments [0, {m}) of {p.n_slices}: device seconds are the minimum "
                 "of three runs after a warm-up, spread = (max - min) / min of the three; all runs in one process")
    lines.append(f"{'storage':>9} {'scaling':>8} {'slice_batch':>11} {'device s':>9} {'spread':>7} {'None / this':>11} "
                 f"{'launches':>9} {'reduce':>7} {'peak bytes':>11} {'GMAC/s':>8} {'bits equal None':>15}")
    for st, sc in ((None, None), ("bfloat16", None), ("float16", "tensor")):
        base = t_base = None
        for B in batches:
            call = lambda B=B: ctr.contract(r0.path, tn.ts_inds, leaves, tn.output_inds, slices=r0.slices,  # noqa: E731
                                            slice_range=(0, m), storage=st, scaling=sc, slice_batch=B)
            r = call()
            times = [call().device_s for _ in range(3)]
            t = min(times)
            if B is None:
                base, t_base = r.array, t
            same = np.array_equal(np.ravel(r.array).view(np.uint32), np.ravel(base).view(np.uint32))
            lines.append(f"{str(st):>9} {str(sc):>8} {str(B):>11} {t:9.4f} {(max(times) - t) / t:7.3f} {t_base / t:11.2f} "
                         f"{r.launches:9d} {r.batch_launches:7d} {r.peak_device_bytes:11d} {r.macs / t / 1e9:8.2f} "
                         f"{str(bool(same)):>15}")
            print(lines[-1], flush=True)
            del r


def path_kernel(lines, depth, max_width, max_slices):
    """A whole assignment per workgroup on the sliced Sycamore amplitude of the storage leg, complex64: the unfused run,
    slice_batch=64 and path_kernel 64, 256 and 1024, all in this process: device time (the minimum and the spread of three
    runs after a warm-up), launches, memory and rate per setting, and the largest relative difference of an element to
    the unfused run, which must be 0."""
    lines.append("")
    ts, d, o = syn.sycamore53_tn(depth=depth)
    tn0 = tnmod.TensorNetwork([tnmod.Tensor(xs, [d] * len(xs)) for xs in ts], output_inds=o)
    tn, res = Optimizer(method="sa", max_width=max_width, seed=0).optimize(tn0, betas=(0, 50), n_steps=200, n_runs=256)
    r0 = res[0]
    rng = np.random.RandomState(2)
    n_inds = len({x for xs in ts for x in xs})
    scale = 2.0 ** (-n_inds / (2 * len(ts)))  # (as in the storage leg: the amplitude stays near 1)
    arrays = [(_rand(tuple(d for _ in xs), np.complex64, rng) * scale).astype(np.complex64) for xs in ts]
    fused = ctr.contract(tn.tags["fuse_path"], tn0.ts_inds, arrays, tn0.output_inds)
    leaves = fused.array if isinstance(fused.array, list) else [fused.array]
    p = ctr.plan(r0.path, tn.ts_inds, [a.shape for a in leaves], tn.output_inds, slices=r0.slices)
    m = min(p.n_slices, max_slices)
    big = max(op["H"] * op["M"] * op["N"] * op["K"] for op in p.ops)
    lines.append(f"## path_kernel, sliced Sycamore-53 amplitude, depth {depth}, complex64, max_width {max_width}, cost "
                 f"{r0.cost}, {len(r0.path)} steps, largest step {big} MACs, arena {p.arena_elems} elements, assignments "
                 f"[0, {m}) of {p.n_slices}: device seconds are the minimum of three runs after a warm-up, spread = "
                 "(max - min) / min of the three; all runs in one process")
    lines.append(f"{'setting':>18} {'device s':>9} {'spread':>7} {'None / this':>11} {'us / slice':>10} {'launches':>9} "
                 f"{'path, reduce':>14} {'peak bytes':>11} {'GMAC/s':>8} {'max rel. diff to None':>21}")
    base = t_base = None
    times_of = {}
    for name, kw in (("None", dict()), ("slice_batch=64", dict(slice_batch=64)), ("path_kernel=64", dict(path_kernel=64)),
                     ("path_kernel=256", dict(path_kernel=256)), ("path_kernel=1024", dict(path_kernel=1024))):
        call = lambda kw=kw: ctr.contract(r0.path, tn.ts_inds, leaves, tn.output_inds, slices=r0.slices,  # noqa: E731
                                          slice_range=(0, m), **kw)
        r = call()
        times = [call().device_s for _ in range(3)]
        t = times_of[name] = min(times)
        if base is None:
            base, t_base = r.array, t
        with np.errstate(divide="ignore", invalid="ignore"):
            diff = float(np.nanmax(np.where(r.array == base, 0.0, np.abs(r.array - base) / np.abs(base))))
        same = np.array_equal(np.ravel(r.array).view(np.uint32), np.ravel(base).view(np.uint32))
        lines.append(f"{name:>18} {t:9.4f} {(max(times) - t) / t:7.3f} {t_base / t:11.2f} {t / m * 1e6:10.2f} {r.launches:9d} "
                     f"{str(r.path_launches):>14} {r.peak_device_bytes:11d} {r.macs / t / 1e9:8.2f} "
                     f"{diff:21.2e}{'' if same else '  (bits differ)'}")
        print(lines[-1], flush=True)
        del r
    a, b = times_of["slice_batch=64"], times_of["path_kernel=1024"]
    lines.append(f"  path_kernel=1024 against slice_batch=64: {a:.4f} s / {b:.4f} s = {a / b:.2f}"
                 f"{'' if b < a else ' -- NOT faster than slice_batch=64 on this leg'}")
    print(lines[-1], flush=True)


def hoist(lines, depth, max_width, max_slices):
    """Slice-independent steps once per call on the sliced Sycamore amplitude of the storage leg, complex64: hoist=None
    against hoist=True, unbatched and with slice_batch=64, all in this process: device time (the minimum and the spread
    of three runs after a warm-up), launches and multiply-adds per setting; every hoisted result is compared bit for
    bit with the run without the keyword."""
    lines.append("")
    ts, d, o = syn.sycamore53_tn(depth=depth)
    tn0 = tnmod.TensorNetwork([tnmod.Tensor(xs, [d] * len(xs)) for xs in ts], output_inds=o)
    tn, res = Optimizer(method="sa", max_width=max_width, seed=0).optimize(tn0, betas=(0, 50), n_steps=200, n_runs=256)
    r0 = res[0]
    rng = np.random.RandomState(2)
    n_inds = len({x for xs in ts for x in xs})
    scale = 2.0 ** (-n_inds / (2 * len(ts)))  # (as in the storage leg: the amplitude stays near 1)
    arrays = [(_rand(tuple(d for _ in xs), np.complex64, rng) * scale).astype(np.complex64) for xs in ts]
    fused = ctr.contract(tn.tags["fuse_path"], tn0.ts_inds, arrays, tn0.output_inds)
    leaves = fused.array if isinstance(fused.array, list) else [fused.array]
    p = ctr.plan(r0.path, tn.ts_inds, [a.shape for a in leaves], tn.output_inds, slices=r0.slices, hoist=True)
    m = min(p.n_slices, max_slices)
    lines.append(f"## hoist, sliced Sycamore-53 amplitude, depth {depth}, complex64, max_width {max_width}, cost {r0.cost}, "
                 f"{len(r0.path)} steps and {len(p.perms)} permutes of which {p.hoisted[0]} steps and {p.hoisted[1]} permutes are "
                 f"hoisted ({p.hoisted_macs} of {p.macs_per_slice} MACs per assignment), {len(p.kept)} kept tensors, arena "
                 f"{p.arena_elems} elements, assignments [0, {m}) of {p.n_slices}: device seconds are the minimum of three runs "
                 "after a warm-up, spread = (max - min) / min of the three; all runs in one process")
    lines.append(f"{'setting':>28} {'device s':>9} {'spread':>7} {'None / this':>11} {'us / slice':>10} {'launches':>9} "
                 f"{'MACs':>14} {'peak bytes':>11} {'bits equal None':>15}")
    for B in (None, 64):
        base = t_base = None
        for h in (None, True):
            call = lambda B=B, h=h: ctr.contract(r0.path, tn.ts_inds, leaves, tn.output_inds, slices=r0.slices,  # noqa: E731
                                                 slice_range=(0, m), slice_batch=B, hoist=h)
            r = call()
            times = [call().device_s for _ in range(3)]
            t = min(times)
            if h is None:
                base, t_base = r.array, t
            same = np.array_equal(np.ravel(r.array).view(np.uint32), np.ravel(base).view(np.uint32))
            lines.append(f"{f'slice_batch={B} hoist={h}':>28} {t:9.4f} {(max(times) - t) / t:7.3f} {t_base / t:11.2f} "
                         f"{t / m * 1e6:10.2f} {r.launches:9d} {r.macs:14d} {r.peak_device_bytes:11d} {str(bool(same)):>15}")
            print(lines[-1], flush=True)
            del r


REUSE_SETTINGS = (("hoist=None", dict()), ("hoist=True", dict(hoist=True)), ("reuse=True", dict(reuse=True)),
                  ("reuse=True slice_order=reuse", dict(reuse=True, slice_order="reuse")),
                  ("reuse=True slice_order=reuse indirect=True", dict(reuse=True, slice_order="reuse", indirect=True)))
# the arithmetic-bound leg of --reuse: (depth, max_width) in the order they are tried, and what an assignment must take
REUSE_BIG = ((10, 18), (12, 20), (12, 22), (14, 24))
REUSE_BIG_MS = 1.0


def _sliced_sycamore(depth, max_width):
    """(tn, the first result of the finite-width optimization, the leaves after the fuse stage): the sliced Sycamore
    amplitude of the storage leg, complex64."""
    ts, d, o = syn.sycamore53_tn(depth=depth)
    tn0 = tnmod.TensorNetwork([tnmod.Tensor(xs, [d] * len(xs)) for xs in ts], output_inds=o)
    tn, res = Optimizer(method="sa", max_width=max_width, seed=0).optimize(tn0, betas=(0, 50), n_steps=200, n_runs=256)
    rng = np.random.RandomState(2)
    n_inds = len({x for xs in ts for x in xs})
    scale = 2.0 ** (-n_inds / (2 * len(ts)))  # (as in the storage leg: the amplitude stays near 1)
    arrays = [(_rand(tuple(d for _ in xs), np.complex64, rng) * scale).astype(np.complex64) for xs in ts]
    fused = ctr.contract(tn.tags["fuse_path"], tn0.ts_inds, arrays, tn0.output_inds)
    return tn, res[0], fused.array if isinstance(fused.array, list) else [fused.array]


def _reuse_rows(lines, tn, r0, leaves, m):
    """The five settings of REUSE_SETTINGS on assignments [0, m), unbatched; every ratio against hoist=True."""
    shapes = [a.shape for a in leaves]
    lines.append(f"{'setting':>44} {'device s':>9} {'spread':>7} {'hoist=True / this':>17} {'ms / slice':>10} {'launches':>9} "
                 f"{'MACs':>15} {'MACs / plain':>12} {'peak bytes':>12} {'reused':>10} {'kept':>5} {'bits equal plain, same order':>28}")
    run = lambda **kw: ctr.contract(r0.path, tn.ts_inds, leaves, tn.output_inds, slices=r0.slices, slice_range=(0, m), **kw)  # noqa: E731
    rows, notes, plain_macs = [], [], None
    for name, kw in REUSE_SETTINGS:
        p = ctr.plan(r0.path, tn.ts_inds, shapes, tn.output_inds, slices=r0.slices, slice_range=(0, m), dtype=np.complex64, **kw)
        r = run(**kw)
        times = [run(**kw).device_s for _ in range(3)]
        t, spread = min(times), (max(times) - min(times)) / min(times)
        # bits: against the run without reuse / hoist under the same order of the sliced indices
        base = run(slice_order=p.slice_inds, **{k: v for k, v in kw.items() if k == "indirect"})
        same = np.array_equal(np.ravel(r.array).view(np.uint32), np.ravel(base.array).view(np.uint32))
        plain_macs = r.macs if plain_macs is None else plain_macs
        rows.append((name, t, spread, r, p, same))
        del base
    t_hoist, s_hoist = rows[1][1], rows[1][2]
    for name, t, spread, r, p, same in rows:
        lines.append(f"{name:>44} {t:9.4f} {spread:7.3f} {t_hoist / t:17.2f} {t / m * 1e3:10.4f} {r.launches:9d} {r.macs:15d} "
                     f"{r.macs / plain_macs:12.3f} {r.peak_device_bytes:12d} {str(r.reused):>10} {len(p.kept):5d} {str(bool(same)):>28}")
        print(lines[-1], flush=True)
        if name.startswith("reuse") and not t * (1 + max(spread, s_hoist)) < t_hoist:
            notes.append(f"  {name}: NOT faster than hoist=True by more than the spread")
    lines.extend(notes)


def reuse(lines, depth, max_width, max_slices):
    """Steps that run only when their slices change, all in this process, unbatched: (a) the sliced Sycamore amplitude of
    the storage leg, launch-bound; (b) the first network of REUSE_BIG whose assignment takes REUSE_BIG_MS milliseconds or
    more under hoist=True (measured here on 8 assignments), on its first 64 assignments.  Device time: the minimum and
    the spread of three runs after a warm-up; the baseline of every ratio is hoist=True."""
    lines.append("")
    tn, r0, leaves = _sliced_sycamore(depth, max_width)
    n = 2 ** len(r0.slices)
    m = min(n, max_slices)
    lines.append(f"## reuse (a), sliced Sycamore-53 amplitude, depth {depth}, complex64, max_width {max_width}, cost {r0.cost}, "
                 f"{len(r0.path)} steps, {len(r0.slices)} sliced indices, assignments [0, {m}) of {n}, unbatched: device seconds "
                 "are the minimum of three runs after a warm-up, spread = (max - min) / min of the three; all runs in one process")
    _reuse_rows(lines, tn, r0, leaves, m)
    del leaves
    for big_depth, big_width in REUSE_BIG:
        tn, r0, leaves = _sliced_sycamore(big_depth, big_width)
        n = 2 ** len(r0.slices)
        probe = ctr.contract(r0.path, tn.ts_inds, leaves, tn.output_inds, slices=r0.slices, slice_range=(0, min(n, 8)), hoist=True)
        probe = ctr.contract(r0.path, tn.ts_inds, leaves, tn.output_inds, slices=r0.slices, slice_range=(0, min(n, 8)), hoist=True)
        ms = probe.device_s / min(n, 8) * 1e3
        lines.append(f"(depth {big_depth}, max_width {big_width}: {len(r0.slices)} sliced indices, {ms:.3f} ms per assignment under "
                     f"hoist=True on the first {min(n, 8)})")
        print(lines[-1], flush=True)
        if ms >= REUSE_BIG_MS or (big_depth, big_width) == REUSE_BIG[-1]:
            break
        del leaves
    m = min(n, 64)
    chosen = (f"the first of {REUSE_BIG} whose assignment takes {REUSE_BIG_MS} ms or more" if ms >= REUSE_BIG_MS else
              f"the last of {REUSE_BIG}: NONE of them takes {REUSE_BIG_MS} ms per assignment, this one {ms:.3f} ms")
    lines.append(f"## reuse (b), sliced Sycamore-53 amplitude, depth {big_depth}, complex64, max_width {big_width}, cost {r0.cost}, "
                 f"{len(r0.path)} steps, {len(r0.slices)} sliced indices, assignments [0, {m}) of {n}, unbatched: {chosen}; "
                 f"the range covers the {int(np.log2(m))} fastest sliced indices of each order only")
    _reuse_rows(lines, tn, r0, leaves, m)


ACCUMULATE_SETTINGS = (("unbatched", dict()), ("slice_batch=64 hoist=True", dict(slice_batch=64, hoist=True)),
                       ("path_kernel=1024", dict(path_kernel=1024)))


def accumulate(lines, depth, max_width, max_slices):
    """The sum over assignments in float64 on the sliced Sycamore amplitude of the storage leg, complex64, all in this
    process: accumulate=None against "float64", unbatched, with slice_batch=64 and hoist=True, and with path_kernel=1024:
    device time (the minimum and the spread of three runs after a warm-up), launches, peak bytes, and the relative error
    by norm of both against the same plan run on the engine in complex128."""
    lines.append("")
    tn, r0, leaves = _sliced_sycamore(depth, max_width)
    n = 2 ** len(r0.slices)
    m = min(n, max_slices)
    run = lambda arrays=leaves, **kw: ctr.contract(r0.path, tn.ts_inds, arrays, tn.output_inds, slices=r0.slices,  # noqa: E731
                                                   slice_range=(0, m), **kw)
    ref = run([a.astype(np.complex128) for a in leaves]).array
    norm = float(np.linalg.norm(np.ravel(ref)))
    lines.append(f"## accumulate, sliced Sycamore-53 amplitude, depth {depth}, complex64, max_width {max_width}, cost {r0.cost}, "
                 f"{len(r0.path)} steps, assignments [0, {m}) of {n}: device seconds are the minimum of three runs after a "
                 "warm-up, spread = (max - min) / min of the three; error = |result - ref| / |ref| by norm, ref the same plan "
                 "run in complex128; all runs in one process")
    lines.append(f"{'setting':>26} {'accumulate':>10} {'device s':>9} {'spread':>7} {'this / None':>11} {'launches':>9} "
                 f"{'peak bytes':>11} {'error':>10} {'bits equal unbatched':>20}")
    first = {}
    for name, kw in ACCUMULATE_SETTINGS:
        t_none = None
        for acc in (None, "float64"):
            r = run(accumulate=acc, **kw)
            times = [run(accumulate=acc, **kw).device_s for _ in range(3)]
            t = min(times)
            t_none = t if acc is None else t_none
            base = first.setdefault(acc, r.array)
            same = np.array_equal(np.ravel(r.array).view(np.uint32), np.ravel(base).view(np.uint32))
            err = float(np.linalg.norm(np.ravel(r.array.astype(np.complex128) - ref))) / norm
            lines.append(f"{name:>26} {str(acc):>10} {t:9.4f} {(max(times) - t) / t:7.3f} {t / t_none:11.3f} {r.launches:9d} "
                         f"{r.peak_device_bytes:11d} {err:10.3e} {str(bool(same)):>20}")
            print(lines[-1], flush=True)
            del r


def indirect(lines, depth, max_width, max_slices):
    """Operands read in place against the permutes they replace, all in this process: the sliced Sycamore amplitude of the
    storage leg, complex64, with slice_batch None and 64, hoist None and True, each with indirect=None and indirect=True;
    and one bandwidth-bound step, a complex64 operand of 2^26 elements whose 26 axes of dimension 2 lie in reversed order,
    summed over four axes in its middle with a vector (the stream class).  Device time: the minimum and the spread of
    three runs after a warm-up; every indirect result is compared bit for bit with the run without the keyword."""
    lines.append("")
    ts, d, o = syn.sycamore53_tn(depth=depth)
    tn0 = tnmod.TensorNetwork([tnmod.Tensor(xs, [d] * len(xs)) for xs in ts], output_inds=o)
    tn, res = Optimizer(method="sa", max_width=max_width, seed=0).optimize(tn0, betas=(0, 50), n_steps=200, n_runs=256)
    r0 = res[0]
    rng = np.random.RandomState(2)
    n_inds = len({x for xs in ts for x in xs})
    scale = 2.0 ** (-n_inds / (2 * len(ts)))  # (as in the storage leg: the amplitude stays near 1)
    arrays = [(_rand(tuple(d for _ in xs), np.complex64, rng) * scale).astype(np.complex64) for xs in ts]
    fused = ctr.contract(tn.tags["fuse_path"], tn0.ts_inds, arrays, tn0.output_inds)
    leaves = fused.array if isinstance(fused.array, list) else [fused.array]
    shapes = [a.shape for a in leaves]
    p0 = ctr.plan(r0.path, tn.ts_inds, shapes, tn.output_inds, slices=r0.slices)
    m = min(p0.n_slices, max_slices)
    folds = {h: ctr.plan(r0.path, tn.ts_inds, shapes, tn.output_inds, slices=r0.slices, hoist=h, indirect=True)
             for h in (None, True)}
    lines.append(f"## indirect, sliced Sycamore-53 amplitude, depth {depth}, complex64, max_width {max_width}, cost {r0.cost}, "
                 f"{len(r0.path)} steps and {len(p0.perms)} permutes, of which indirect=True folds {folds[None].indirect} "
                 f"({folds[True].indirect} beside hoist=True, which runs {folds[True].hoisted[1]} once per call), offset tables "
                 f"{folds[None].ind_maps.size} entries, assignments [0, {m}) of {p0.n_slices}: device seconds are the minimum of "
                 "three runs after a warm-up, spread = (max - min) / min of the three; all runs in one process")
    head = (f"{'setting':>44} {'device s':>9} {'spread':>7} {'None / this':>11} {'us / slice':>10} {'launches':>9} "
            f"{'indirect launches':>18} {'peak bytes':>11} {'bits equal None':>15}")
    lines.append(head)
    notes = []

    def rows(label, call_of, metric=lambda t, r: t / r.n_slices * 1e6):
        base = t_base = spread_base = None
        for ind in (None, True):
            call = lambda ind=ind: call_of(ind)  # noqa: E731
            r = call()
            times = [call().device_s for _ in range(3)]
            t, spread = min(times), (max(times) - min(times)) / min(times)
            if ind is None:
                base, t_base, spread_base = r.array, t, spread
            same = np.array_equal(np.ravel(r.array).view(np.uint32), np.ravel(base).view(np.uint32))
            lines.append(f"{f'{label} indirect={ind}':>44} {t:9.4f} {spread:7.3f} {t_base / t:11.2f} "
                         f"{metric(t, r):10.2f} "
                         f"{r.launches:9d} {str(r.indirect_launches):>18} {r.peak_device_bytes:11d} {str(bool(same)):>15}")
            print(lines[-1], flush=True)
            if ind and t > t_base * (1 + max(spread, spread_base)):
                notes.append(f"  {label}: indirect=True is SLOWER than indirect=None by more than the spread")
            del r

    for B in (None, 64):
        for h in (None, True):
            rows(f"slice_batch={B} hoist={h}",
                 lambda ind, B=B, h=h: ctr.contract(r0.path, tn.ts_inds, leaves, tn.output_inds, slices=r0.slices,
                                                    slice_range=(0, m), slice_batch=B, hoist=h, indirect=ind))
    del leaves, arrays
    # the bandwidth-bound step: X (x25, ..., x0), 2^26 complex64, summed over x13..x10 with Y (x13, ..., x10): M = 2^22
    # around K = 16, N = 1, the stream class; the plain plan permutes X (a read and a write of 512 MiB) before it reads
    # the copy
    nx, ks = 26, (13, 12, 11, 10)
    xs = tuple(f"x{q}" for q in reversed(range(nx)))
    ys = tuple(f"x{q}" for q in ks)
    x, y = _rand((2,) * nx, np.complex64, rng), _rand((2,) * len(ks), np.complex64, rng)
    q = ctr.plan([(0, 1)], [xs, ys], [x.shape, y.shape], dtype=np.complex64, indirect=True)
    op = q.ops[0]
    lines.append(f"## indirect, one bandwidth-bound step: X complex64, 2^{nx} elements, axes of dimension 2 in reversed "
                 "order, "
                 f"Z = sum over {len(ks)} axes in its middle of X Y: M N K = {op['M']} x {op['N']} x {op['K']} (stream class), "
                 f"{q.indirect} operand folded, offset tables {q.ind_maps.size} entries; effective GB/s = (X + Z bytes) / time")
    lines.append(head.replace("us / slice", "      GB/s"))
    moved = x.nbytes + x.nbytes // op["K"]
    rows("reversed 2^26", lambda ind: ctr.contract([(0, 1)], [xs, ys], [x, y], indirect=ind),
         lambda t, r: moved / t / 1e9)
    lines.extend(notes)


def resident(lines, depth, max_width, max_slices, reps=5):
    """What a call costs around its kernels: wall time per call (time.perf_counter, the device synchronised on both sides)
    of contract() and of three ways to use one Contractor, device_s next to it; per setting the minimum of `reps` calls
    after a warm-up and their spread, all settings in this process.  Two legs: the sliced Sycamore amplitude of the
    path-kernel leg under path_kernel=1024, and the bandwidth-bound step of the indirect leg (X of 2^26 complex64)."""
    lines.append("")
    notes = []

    def leg(title, path, ts, leaves, output, kw):
        lines.append(title)
        lines.append(f"{'setting':>46} {'wall s':>10} {'spread':>7} {'contract() / this':>17} {'device s':>10} {'io launches':>12} {'same bytes':>10}")
        shapes = [a.shape for a in leaves]
        tensors = [torch.from_numpy(a).cuda() for a in leaves]
        rows, base = [], None
        with ctr.Contractor(path, ts, shapes, output, dtype=np.complex64, **kw) as c:
            out = torch.empty(tuple(c.plan.shape), dtype=torch.complex64, device="cuda")

            def bound_numpy():
                return c.run()

            def bound_torch():
                return c.run(out=out)

            settings = (("contract()", None, lambda: ctr.contract(path, ts, leaves, output, **kw)),
                        ("Contractor.run(numpy arrays)", None, lambda: c.run(leaves)),
                        ("Contractor.run(), leaves bound from numpy", lambda: c.bind(dict(enumerate(leaves))), bound_numpy),
                        ("Contractor.run(out=tensor), bound from torch", lambda: c.bind(dict(enumerate(tensors))), bound_torch))
            for name, before, call in settings:
                if before is not None:
                    before()
                r = call()  # warm-up
                times, dev = [], []
                for _ in range(reps):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    r = call()
                    torch.cuda.synchronize()
                    times.append(time.perf_counter() - t0)
                    dev.append(r.device_s)
                got = r.array if isinstance(r.array, np.ndarray) else r.array.cpu().numpy()
                if base is None:
                    base = got
                same = np.array_equal(np.ravel(got).view(np.uint32), np.ravel(base).view(np.uint32))
                rows.append((name, min(times), (max(times) - min(times)) / min(times), min(dev), c.io_launches, same))
        t_base, s_base = rows[0][1], rows[0][2]
        for name, t, spread, dev, io, same in rows:
            lines.append(f"{name:>46} {t:10.6f} {spread:7.3f} {t_base / t:17.2f} {dev:10.6f} {str(io):>12} {str(same):>10}")
            print(lines[-1], flush=True)
            if t > t_base * (1 + max(spread, s_base)):
                notes.append(f"  {name}: SLOWER per call than contract() by more than the larger of the two spreads")
        del tensors, out

    tn, r0, leaves = _sliced_sycamore(depth, max_width)
    p = ctr.plan(r0.path, tn.ts_inds, [a.shape for a in leaves], tn.output_inds, slices=r0.slices)
    m = min(p.n_slices, max_slices)
    leg(f"## resident, sliced Sycamore-53 amplitude, depth {depth}, complex64, max_width {max_width}, cost {r0.cost}, "
        f"{len(leaves)} leaves, {len(r0.path)} steps, assignments [0, {m}) of {p.n_slices}, path_kernel=1024: wall seconds per call "
        f"(perf_counter, device synchronised on both sides), the minimum of {reps} calls after a warm-up, spread = (max - min) / min; "
        "device s: the minimum device_s of the same calls; all settings in one process",
        r0.path, tn.ts_inds, leaves, tn.output_inds, dict(slices=r0.slices, slice_range=(0, m), path_kernel=1024))
    del leaves
    rng = np.random.RandomState(2)
    nx, ks = 26, (13, 12, 11, 10)
    xs = tuple(f"x{q}" for q in reversed(range(nx)))
    ys = tuple(f"x{q}" for q in ks)
    x, y = _rand((2,) * nx, np.complex64, rng), _rand((2,) * len(ks), np.complex64, rng)
    lines.append("")
    leg(f"## resident, one bandwidth-bound step: X complex64, 2^{nx} elements ({x.nbytes >> 20} MiB), axes of dimension 2 in "
        f"reversed order, Z = sum over {len(ks)} axes in its middle of X Y, indirect=True: the same columns",
        [(0, 1)], [xs, ys], [x, y], None, dict(indirect=True))
    lines.extend(notes)


def many(lines, depth, max_width, max_slices, reps=5, stacked=8):
    """Contractor.run_many against the loop of Contractor.run() over the same leaf sets on the same Contractor, which is
    what there is without it: the sliced Sycamore amplitude of the path-kernel leg, complex64, path_kernel=1024, every
    leaf a torch tensor on the device, the results written into one tensor on the device.  The stacked leaves are the
    `stacked` leaves of fewest elements (ties by leaf number), the others are bound.  Wall seconds (perf_counter, the
    device synchronised on both sides), the minimum of `reps` calls after a warm-up and their spread, both sides of a
    row pair in this process.  Two legs: (a) one assignment per set, 1024 sets -- bound by launches and by the calls;
    (b) every assignment, 8 sets -- bound by the device."""
    lines.append("")
    tn, r0, leaves = _sliced_sycamore(depth, max_width)
    shapes = [a.shape for a in leaves]
    p = ctr.plan(r0.path, tn.ts_inds, shapes, tn.output_inds, slices=r0.slices)
    m = min(p.n_slices, max_slices)
    order = sorted(range(len(leaves)), key=lambda t: (leaves[t].size, t))[:stacked]
    lines.append(f"## run_many, sliced Sycamore-53 amplitude, depth {depth}, complex64, max_width {max_width}, cost {r0.cost}, "
                 f"{len(leaves)} leaves, {len(r0.path)} steps, path_kernel=1024; stacked: the {len(order)} leaves of fewest elements "
                 f"{order} ({sum(leaves[t].size for t in order)} elements per set), the others bound; torch tensors in, one "
                 f"tensor out; wall seconds (perf_counter, device synchronised on both sides), the minimum of {reps} calls after a "
                 "warm-up, spread = (max - min) / min; a loop row is R calls of run(); both rows of a leg in one process")
    lines.append(f"{'leg':>34} {'setting':>24} {'wall s':>10} {'spread':>7} {'us / set':>10} {'loop / this':>11} {'launches':>9} "
                 f"{'peak bytes':>12} {'same bytes':>10}")
    rng = np.random.RandomState(3)
    notes = []
    for leg, rng_, R in (("(a) assignments [0, 1), R = 1024", (0, 1), 1024), (f"(b) assignments [0, {m}), R = 8", (0, m), 8)):
        stacks = {t: torch.from_numpy(np.stack([leaves[t] * np.complex64(np.exp(2j * np.pi * rng.uniform())) for _ in range(R)])).cuda()
                  for t in order}
        with ctr.Contractor(r0.path, tn.ts_inds, shapes, tn.output_inds, dtype=np.complex64, slices=r0.slices, slice_range=rng_,
                            path_kernel=1024) as c:
            c.bind({t: torch.from_numpy(a).cuda() for t, a in enumerate(leaves) if t not in stacks})
            outs = [torch.zeros((R,) + tuple(c.plan.shape), dtype=torch.complex64, device="cuda") for _ in range(2)]
            seen = {}

            def loop():
                n = 0
                for i in range(R):
                    r = c.run({t: s[i] for t, s in stacks.items()}, out=outs[0][i])
                    n += r.launches
                seen.setdefault("loop", (n, r.peak_device_bytes))  # (the memory before run_many grows the handle)

            def batched():
                r = c.run_many(stacks, group=1024, out=outs[1])
                seen["many"] = (r.launches, r.peak_device_bytes)

            rows = []
            for name, key, call in ((f"{R} x run()", "loop", loop), ("run_many(group=1024)", "many", batched)):
                call()  # warm-up
                times = []
                for _ in range(reps):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    call()
                    torch.cuda.synchronize()
                    times.append(time.perf_counter() - t0)
                rows.append((name, min(times), (max(times) - min(times)) / min(times), seen[key]))
            same = bool(torch.equal(torch.view_as_real(outs[0]), torch.view_as_real(outs[1])))
        (_, t_loop, s_loop, _), (_, t_many, s_many, _) = rows
        for name, t, spread, (launches, peak) in rows:
            lines.append(f"{leg:>34} {name:>24} {t:10.6f} {spread:7.3f} {t / R * 1e6:10.2f} {t_loop / t:11.2f} {launches:9d} "
                         f"{peak:12d} {str(same):>10}")
            print(lines[-1], flush=True)
        wider = max(s_loop, s_many)
        if t_many * (1 + wider) < t_loop:
            notes.append(f"  {leg}: run_many is faster than the loop by more than the larger spread ({wider:.3f})")
        elif t_many > t_loop * (1 + wider):
            notes.append(f"  {leg}: run_many is SLOWER than the loop by more than the larger spread ({wider:.3f})")
        else:
            notes.append(f"  {leg}: run_many and the loop are within the larger spread ({wider:.3f}) of each other")
        if not same:
            notes.append(f"  {leg}: THE BYTES OF run_many DIFFER FROM THE LOOP'S")
        del stacks, outs
    lines.extend(notes)
    print("\n".join(notes), flush=True)


def sample_joint(lines, n_qubits=8, n_gates=40, n_samples=4096, reps=5):
    """The walk of `sample`'s circuit with every CZ replaced by fSim(pi / 2, pi / 6), a 2-qubit gate that draws (as numpy
    computes it: cos(pi / 2) is 6e-17 and the phase's modulus is not 1 to the last bit, so it is no permutation with phases
    for `classical_table`), through sampling.Sampler(max_gate_qubits=2), two ways on the same Contractors in one process.
    (a) Sampler.sample: run_walkers + choose_joint per fSim, on the device.  (b) the best a caller can write without the
    joint-draw kernel: the same Walkers, run_walkers, `choose` for the 1-qubit gates, and for an fSim the four amplitudes
    per walker from `walker_outputs`, the tails and the draw in torch on the device (torch's own generator), the two new
    bits written back through Walkers.bits / Walkers.write.  Wall seconds as in `sample`."""
    from tnco_amd import contraction, sampling
    lines.append("")
    rng = np.random.RandomState(17)
    theta, phi = np.pi / 2, np.pi / 6
    fsim = np.array([[1, 0, 0, 0], [0, np.cos(theta), -1j * np.sin(theta), 0], [0, -1j * np.sin(theta), np.cos(theta), 0],
                     [0, 0, 0, np.exp(-1j * phi)]]).astype(np.complex64)

    def unitary():
        q, r = np.linalg.qr(rng.normal(size=(2, 2)) + 1j * rng.normal(size=(2, 2)))
        return (q * (np.diag(r) / np.abs(np.diag(r)))).astype(np.complex64)

    circuit = [(unitary(), (q,)) for q in range(n_qubits)]
    while len(circuit) < n_gates:
        if rng.randint(0, 2):
            circuit.append((unitary(), (int(rng.randint(0, n_qubits)),)))
        else:
            a, b = rng.choice(n_qubits, 2, replace=False)
            circuit.append((fsim, (int(a), int(b))))
    with sampling.Sampler(circuit, seed=0, max_gate_qubits=2) as s:
        joint = [g for g in sorted(s.contractors) if len(s.gates[g][1]) == 2]
        if len(s.contractors) != n_gates:
            raise RuntimeError("a gate of the circuit does not draw.")
        lines.append(f"## sampling with joint draws: {n_qubits} qubits, {n_gates} gates ({n_gates - len(joint)} 1-qubit gates, {len(joint)} "
                     f"fSim(pi/2, pi/6), each a drawing gate of 2 qubits), {n_samples} samples, complex64, path_kernel=group=1024, "
                     f"one Contractor per gate (infinite-memory SA, 8 runs x 100 sweeps); wall seconds of one walk (perf_counter, "
                     f"device synchronised), the minimum of {reps} after a warm-up, spread = (max - min) / min; both rows in one "
                     "process on the same Contractors")
        gen = torch.Generator(device="cuda")
        gen.manual_seed(0)

        def with_kernel():
            return s.sample(n_samples)[0]

        def with_torch():
            with contraction.Walkers(n_samples, n_qubits, seed=0, device=s.device) as w:
                for g, (_, qs) in enumerate(s.gates):
                    c, closing = s.contractors[g]
                    c.run_walkers(w, closing, group=s.group)
                    if len(qs) == 1:
                        c.choose(w, qs[0], g)
                        continue
                    axes = [1 + c.plan.inds.index(x) for x in s.open_inds[g]]
                    amp = torch.from_numpy(c.walker_outputs(w)).to("cuda").permute(0, *axes).reshape(n_samples, -1)
                    p = amp.real.double() ** 2 + amp.imag.double() ** 2
                    tail = p.flip(1).cumsum(1).flip(1)
                    u = torch.rand(n_samples, dtype=torch.float64, device="cuda", generator=gen)
                    v = ((u * tail[:, 0])[:, None] < tail[:, 1:]).sum(1).cpu().numpy()  # (the tails do not rise with v)
                    bits = w.bits
                    for j, q in enumerate(qs):
                        bits[:, q] = (v >> (len(qs) - 1 - j)) & 1
                    w.write(bits)
                return sampling.tally(w.bits)

        rows = []
        for name, call in (("Sampler.sample (choose_joint)", with_kernel), ("walker_outputs + torch draw", with_torch)):
            hits = call()  # warm-up
            times = []
            for _ in range(reps):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                call()
                torch.cuda.synchronize()
                times.append(time.perf_counter() - t0)
            rows.append((name, min(times), (max(times) - min(times)) / min(times), len(hits)))
    lines.append(f"{'way':>32} {'wall s':>10} {'spread':>7} {'us / sample':>12} {'ms / gate':>10} {'bitstrings seen':>16}")
    for name, t, spread, seen in rows:
        lines.append(f"{name:>32} {t:10.6f} {spread:7.3f} {t / n_samples * 1e6:12.3f} {t / n_gates * 1e3:10.4f} {seen:16d}")
    (_, t_new, s_new, _), (_, t_old, s_old, _) = rows
    both = s_new + s_old
    lines.append(f"  torch draw / choose_joint = {t_old / t_new:.2f}x (the two spreads together: {both:.3f})")
    if t_new > t_old * (1 + both):
        lines.append("  THE KERNEL'S WALK IS SLOWER than the torch draw's by more than the two spreads")
    elif t_new * (1 + both) < t_old:
        lines.append("  the kernel's walk is faster than the torch draw's by more than the two spreads")
    else:
        lines.append("  the two walks are within their spreads of each other")
    print("\n".join(lines[-6:]), flush=True)


def sample(lines, n_qubits=8, n_gates=40, n_samples=4096, reps=5):
    """One walk of a fixed random circuit (1-qubit unitaries and CZs, seeded) for `n_samples` samples, two ways, on the
    same Contractors (one per 1-qubit gate, the Sampler's) in one process.  (a) sampling.Sampler: Walkers on the device,
    run_walkers + choose per 1-qubit gate, permute per CZ, one read of the bits.  (b) the best a caller can write with
    run_many alone: the bits a torch tensor on the device, per 1-qubit gate the one-hot stacks of the closing leaves
    built by torch indexing, one run_many with the measured qubit's index open (two amplitudes per walker), the choice
    in torch (torch's own generator); per CZ nothing (it moves no bit), one copy of the bits to the host at the end.
    Wall seconds (perf_counter, device synchronised), the minimum of `reps` walks after a warm-up and the spread."""
    from tnco_amd import sampling
    lines.append("")
    rng = np.random.RandomState(17)
    cz = np.diag([1, 1, 1, -1]).astype(np.complex64)

    def unitary():
        q, r = np.linalg.qr(rng.normal(size=(2, 2)) + 1j * rng.normal(size=(2, 2)))
        return (q * (np.diag(r) / np.abs(np.diag(r)))).astype(np.complex64)

    circuit = [(unitary(), (q,)) for q in range(n_qubits)]
    while len(circuit) < n_gates:
        if rng.randint(0, 2):
            circuit.append((unitary(), (int(rng.randint(0, n_qubits)),)))
        else:
            a, b = rng.choice(n_qubits, 2, replace=False)
            circuit.append((cz, (int(a), int(b))))
    with sampling.Sampler(circuit, seed=0) as s:
        drawing = sorted(s.contractors)
        lines.append(f"## sampling: {n_qubits} qubits, {n_gates} gates ({len(drawing)} 1-qubit gates, {n_gates - len(drawing)} CZ), "
                     f"{n_samples} samples, complex64, path_kernel=group=1024, one Contractor per 1-qubit gate (infinite-memory SA, "
                     f"8 runs x 100 sweeps); wall seconds of one walk (perf_counter, device synchronised), the minimum of {reps} "
                     "after a warm-up, spread = (max - min) / min; both rows in one process on the same Contractors")
        eye = torch.eye(2, dtype=torch.complex64, device="cuda")
        gen = torch.Generator(device="cuda")
        gen.manual_seed(0)

        def with_walkers():
            return s.sample(n_samples)[0]

        def with_run_many():
            bits = torch.zeros((n_samples, n_qubits), dtype=torch.long, device="cuda")
            for g in drawing:
                c, closing = s.contractors[g]
                q = s.gates[g][1][0]
                if closing:
                    amp = c.run_many({t: eye[bits[:, x]] for t, x in closing.items()}, group=1024).array
                else:  # (nothing depends on the walker: one run for all)
                    amp = c.run(out=torch.empty(2, dtype=torch.complex64, device="cuda")).array.expand(n_samples, 2)
                p = amp.real.double() ** 2 + amp.imag.double() ** 2
                u = torch.rand(n_samples, dtype=torch.float64, device="cuda", generator=gen)
                bits[:, q] = (u * (p[:, 0] + p[:, 1]) < p[:, 1]).long()
            return sampling.tally(bits.cpu().numpy())

        rows = []
        for name, call in (("Sampler.sample (walkers)", with_walkers), ("run_many + torch (no walkers)", with_run_many)):
            hits = call()  # warm-up
            times = []
            for _ in range(reps):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                call()
                torch.cuda.synchronize()
                times.append(time.perf_counter() - t0)
            rows.append((name, min(times), (max(times) - min(times)) / min(times), len(hits)))
    lines.append(f"{'way':>32} {'wall s':>10} {'spread':>7} {'us / sample':>12} {'ms / 1-qubit gate':>18} {'bitstrings seen':>16}")
    for name, t, spread, seen in rows:
        lines.append(f"{name:>32} {t:10.6f} {spread:7.3f} {t / n_samples * 1e6:12.3f} {t / len(drawing) * 1e3:18.4f} {seen:16d}")
    (_, t_new, s_new, _), (_, t_old, s_old, _) = rows
    both = s_new + s_old
    lines.append(f"  run_many loop / walkers = {t_old / t_new:.2f}x (the two spreads together: {both:.3f})")
    if t_new > t_old * (1 + both):
        lines.append("  THE WALKERS ARE SLOWER than the run_many loop by more than the two spreads")
    elif t_new * (1 + both) < t_old:
        lines.append("  the walkers are faster than the run_many loop by more than the two spreads")
    else:
        lines.append("  the walkers and the run_many loop are within the two spreads of each other")
    print("\n".join(lines[-5:]), flush=True)


def compute(lines, n, depth, max_width, max_slices):
    """The compute mode against the plain engine in the same process: the large square step with compute=None (the tiled
    LDS kernel, the yardstick), compute="bf16x3" (ct_split_tiled_kernel) and storage="bfloat16" (ct_mfma_tiled_kernel), and
    the sliced Sycamore amplitude of the storage leg with compute=None and "bf16x3"."""
    lines.append("")
    lines.append(f"## compute mode, large square step M = N = K = {n}: float32 / complex64 storage, every product as three "
                 "bfloat16 products on the matrix cores (ct_split_tiled_kernel), against compute=None (the tiled LDS kernel) "
                 "and storage=\"bfloat16\" (ct_mfma_tiled_kernel) in one process; seconds: the minimum of four runs")
    lines.append(f"{'dtype':>10} {'mode':>20} {'engine s':>10} {'TFLOP/s':>9} {'None / this':>12} {'rel. error to float64':>22}")
    rng = np.random.RandomState(6)
    for dt in (np.float32, np.complex64):
        x, y = _rand((n, n), dt, rng), _rand((n, n), dt, rng)
        fl = FLOPS_PER_MAC[dt] * n ** 3
        ref = x.astype(np.complex128 if np.dtype(dt).kind == "c" else np.float64) @ y
        t_base = None
        for name, kw in (("compute=None", dict()), ("compute=bf16x3", dict(compute="bf16x3")),
                         ("storage=bfloat16", dict(storage="bfloat16"))):
            call = lambda kw=kw: ctr.contract([(0, 1)], [("i", "k"), ("k", "j")], [x, y], **kw)  # noqa: E731
            r = call()
            t = min(r.device_s, _engine_time(call))
            t_base = t if t_base is None else t_base
            err = float(np.linalg.norm(r.array - ref) / np.linalg.norm(ref))
            lines.append(f"{np.dtype(dt).name:>10} {name:>20} {t:10.5f} {fl / t / 1e12:9.1f} {t_base / t:12.2f} {err:22.2e}")
            print(lines[-1], flush=True)
            del r
        del ref, x, y
    ts, d, o = syn.sycamore53_tn(depth=depth)
    tn0 = tnmod.TensorNetwork([tnmod.Tensor(xs, [d] * len(xs)) for xs in ts], output_inds=o)
    tn, res = Optimizer(method="sa", max_width=max_width, seed=0).optimize(tn0, betas=(0, 50), n_steps=200, n_runs=256)
    r0 = res[0]
    rng = np.random.RandomState(2)
    n_inds = len({x for xs in ts for x in xs})
    scale = 2.0 ** (-n_inds / (2 * len(ts)))  # (as in the storage leg: the amplitude stays near 1)
    arrays = [(_rand(tuple(d for _ in xs), np.complex64, rng) * scale).astype(np.complex64) for xs in ts]
    fused = ctr.contract(tn.tags["fuse_path"], tn0.ts_inds, arrays, tn0.output_inds)
    leaves = fused.array if isinstance(fused.array, list) else [fused.array]
    p = ctr.plan(r0.path, tn.ts_inds, [a.shape for a in leaves], tn.output_inds, slices=r0.slices)
    m = min(p.n_slices, max_slices)
    run = lambda c: ctr.contract(r0.path, tn.ts_inds, leaves, tn.output_inds, slices=r0.slices, slice_range=(0, m),  # noqa: E731
                                 compute=c)
    run(None)
    a, b = run(None), run("bf16x3")
    err = float(np.linalg.norm(np.ravel(b.array - a.array)) / np.linalg.norm(np.ravel(a.array)))
    tiled = sum(1 for op in p.ops if op["M"] >= 64 and op["N"] >= 64 and op["K"] > 32)
    lines.append(f"## compute mode, sliced Sycamore-53 amplitude, depth {depth}, complex64, max_width {max_width}, "
                 f"assignments [0, {m}), {tiled} of {len(p.ops)} steps of the tiled class: compute=None: device "
                 f"{a.device_s:.3f} s; compute=\"bf16x3\": device {b.device_s:.3f} s, {b.split_launches} launches of the "
                 f"split kernel of {b.launches}, None / this {a.device_s / b.device_s:.2f}, relative difference to the "
                 f"compute=None run {err:.2e}, peak device bytes {b.peak_device_bytes} (None: {a.peak_device_bytes})")
    print(lines[-1], flush=True)


def matrix(lines, n, block=64):
    """The matrix mode against the plain engine in the same process: the large square step in the four dtypes with
    compute=None (the tiled LDS kernel, the yardstick) and compute="matrix" (ct_matrix_tiled_kernel); in float32 and
    complex64 also compute="bf16x3" and storage="bfloat16"; torch.tensordot on the same operands.  Device time: the
    minimum and the spread of three runs after a warm-up.  Every row carries the largest difference to the host product
    in float64 / complex128 on the leading block x block of the result, relative to the largest modulus there."""
    lines.append("")
    lines.append(f"## matrix mode, large square step M = N = K = {n}: the arrays' own dtype on the matrix cores "
                 "(ct_matrix_tiled_kernel: v_mfma_f32_16x16x4_f32 / v_mfma_f64_16x16x4_f64) against compute=None (the tiled "
                 "LDS kernel), the other matrix-core modes and torch.tensordot, all in one process; device seconds: the "
                 "minimum of three runs after a warm-up, spread = (max - min) / min of the three; error: max |got - ref| / "
                 f"max |ref| over the leading {block} x {block} block of the result, ref the host product in float64 / complex128")
    lines.append(f"{'dtype':>10} {'mode':>18} {'device s':>9} {'spread':>7} {'TFLOP/s':>8} {'None / this':>11} {'torch / this':>12} "
                 f"{'error':>9}")
    rng = np.random.RandomState(7)
    notes = []
    for dt in (np.float32, np.float64, np.complex64, np.complex128):
        x, y = _rand((n, n), dt, rng), _rand((n, n), dt, rng)
        fl = FLOPS_PER_MAC[dt] * n ** 3
        wide = np.complex128 if np.dtype(dt).kind == "c" else np.float64
        ref = x[:block].astype(wide) @ y[:, :block].astype(wide)
        tx, ty = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
        t_torch = _torch_time(lambda: torch.tensordot(tx, ty, dims=([1], [0])))
        del tx, ty
        torch.cuda.empty_cache()
        modes = [("compute=None", dict()), ("compute=matrix", dict(compute="matrix"))]
        if np.dtype(dt).itemsize // (2 if np.dtype(dt).kind == "c" else 1) == 4:
            modes += [("compute=bf16x3", dict(compute="bf16x3")), ("storage=bfloat16", dict(storage="bfloat16"))]
        t_base = spread_base = None
        for name, kw in modes:
            call = lambda kw=kw: ctr.contract([(0, 1)], [("i", "k"), ("k", "j")], [x, y], **kw)  # noqa: E731
            r = call()
            times = [call().device_s for _ in range(3)]
            t, spread = min(times), (max(times) - min(times)) / min(times)
            if t_base is None:
                t_base, spread_base = t, spread
            err = float(np.abs(r.array[:block, :block] - ref).max() / np.abs(ref).max())
            lines.append(f"{np.dtype(dt).name:>10} {name:>18} {t:9.5f} {spread:7.3f} {fl / t / 1e12:8.1f} {t_base / t:11.2f} "
                         f"{t_torch / t:12.2f} {err:9.2e}")
            print(lines[-1], flush=True)
            if name == "compute=matrix" and not t * (1 + max(spread, spread_base)) < t_base:
                notes.append(f"  {np.dtype(dt).name}: compute=matrix is NOT faster than compute=None by more than the spread")
            del r
        lines.append(f"{np.dtype(dt).name:>10} {'torch.tensordot':>18} {t_torch:9.5f} {'':>7} {fl / t_torch / 1e12:8.1f} "
                     f"{t_base / t_torch:11.2f} {1.0:12.2f} {'':>9}")
        print(lines[-1], flush=True)
        del ref, x, y
    lines.extend(notes)


def projections(lines, depth, counts, loop_max):
    """P amplitudes per call.  The network: the circuit without its 53 <x| tensors, the open wires its output and
    sparse indices.  The largest depth <= `depth` whose unsliced plan fits the free device memory at every P is used."""
    lines.append("")
    free = torch.cuda.mem_get_info()[0]
    rng = np.random.RandomState(3)
    while True:
        ts, d, _ = syn.sycamore53_tn(depth=depth)
        ts, out = [tuple(x) for x in ts[:-53]], [x[0] for x in ts[-53:]]
        tn0 = tnmod.TensorNetwork([tnmod.Tensor(xs, [d] * len(xs)) for xs in ts], output_inds=out, sparse_inds=out)
        sparse = sorted(out, key=str)
        arrays = [_rand(tuple(d for _ in xs), np.complex64, rng) for xs in ts]
        runs = []
        for P in counts:
            tn, res = Optimizer(method="sa", seed=0).optimize(tn0, betas=(0, 50), n_steps=200, n_runs=256, n_projs=P,
                                                              fuse=None, decompose_hyper_inds=False)
            projs = rng.randint(0, 2, (P, 53))
            p = ctr.plan(res[0].path, tn.ts_inds, [a.shape for a in arrays], tn.output_inds, dtype=np.complex64,
                         sparse_inds=sparse, projs=projs)
            runs.append((P, res[0], projs, p))
        need = max(p.peak_device_bytes for *_, p in runs)
        if need <= 0.9 * free or depth <= 2:
            break
        lines.append(f"(depth {depth}: the unsliced plan needs {need} bytes, {free} are free: two cycles fewer)")
        depth -= 2
    lines.append(f"## P bitstring amplitudes of Sycamore-53, depth {depth}, complex64, in one projected call: {len(ts)} "
                 f"tensors, 53 sparse output indices, infinite-memory SA per P (256 runs x 200 sweeps); loop: contract() "
                 f"per bitstring over leaves indexed at it, same path")
    for P, r0, projs, p in runs:
        call = lambda: ctr.contract(r0.path, tn0.ts_inds, arrays, out, sparse_inds=sparse, projs=projs)  # noqa: E731
        r = call()
        t_p = min(r.device_s, _engine_time(call, reps=2))
        # the loop a user writes without projections, on min(P, loop_max) bitstrings, scaled linearly to P
        n_loop = min(P, loop_max)
        t_l = macs_l = launches_l = 0
        worst = 0.0
        for k in range(n_loop):
            bits = dict(zip(sparse, projs[k]))
            fixed = [tuple(x for x in xs if x not in bits) for xs in ts]
            leaves = [a[tuple(bits[x] if x in bits else slice(None) for x in xs)] for a, xs in zip(arrays, ts)]
            q = ctr.contract(r0.path, fixed, leaves, ())
            t_l, macs_l, launches_l = t_l + q.device_s, macs_l + q.macs, launches_l + q.launches
            got, ref = r.array[k], q.array
            worst = max(worst, float(abs(got - ref) / max(abs(ref), 1e-30)))
        scale = P / n_loop
        stream = [op for op in p.ops if not op["folded"] and (op["R"] > 1 or op["a_map"] is not None
                                                              or op["b_map"] is not None)]
        lines.append(f"  P = {P}: cost {r0.cost}, projected call device {t_p:.5f} s, MACs {r.macs}, "
                     f"{r.macs / t_p / 1e9:.1f} GMAC/s, peak device bytes {r.peak_device_bytes}; launches "
                     f"{dict(zip(ctr.KERNEL_PATHS, r.kernel_launches))} {dict(zip(ctr.ROW_KERNEL_PATHS, r.row_kernel_launches))}"
                     f" ({len(stream)} steps with rows, most rows {max(op['R'] for op in p.ops if not op['folded'])})")
        lines.append(f"    loop of contract(): {n_loop} bitstrings measured, device {t_l:.5f} s, {launches_l} launches, MACs "
                     f"{macs_l}; scaled x{scale:g} to P{' (scaled)' if scale != 1 else ''}: {t_l * scale:.5f} s; "
                     f"loop / projected = {t_l * scale / t_p:.1f}x; largest relative difference of an amplitude {worst:.2e}")
    print("\n".join(lines[-1 - 2 * len(runs):]), flush=True)
    return runs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "contract_timing.txt"))
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--depth", type=int, default=8)
    ap.add_argument("--max-width", type=float, default=14)
    ap.add_argument("--max-slices", type=int, default=4096)
    ap.add_argument("--projs", action="store_true", help="only the projections leg, appended to --out")
    ap.add_argument("--storage", action="store_true", help="only the storage-mode leg, appended to --out")
    ap.add_argument("--scaling", action="store_true", help="only the scaling leg, appended to --out")
    ap.add_argument("--slice-batch", action="store_true", help="only the slice-batch leg, appended to --out")
    ap.add_argument("--compute", action="store_true", help="only the compute-mode leg, appended to --out")
    ap.add_argument("--path-kernel", action="store_true", help="only the path-kernel leg, appended to --out")
    ap.add_argument("--hoist", action="store_true", help="only the hoisting leg, appended to --out")
    ap.add_argument("--matrix", action="store_true", help="only the matrix-mode leg, appended to --out")
    ap.add_argument("--indirect", action="store_true", help="only the indirect-operand leg, appended to --out")
    ap.add_argument("--reuse", action="store_true", help="only the reuse leg, appended to --out")
    ap.add_argument("--accumulate", action="store_true", help="only the wide-accumulation leg, appended to --out")
    ap.add_argument("--resident", action="store_true", help="only the resident (Contractor) leg, appended to --out")
    ap.add_argument("--many", action="store_true", help="only the run_many leg, appended to --out")
    ap.add_argument("--sample", action="store_true", help="only the sampling leg, appended to --out")
    ap.add_argument("--sample-joint", action="store_true", help="only the joint-draw sampling leg, appended to --out")
    ap.add_argument("--counts", type=int, nargs="+", default=[64, 1024, 16384])
    ap.add_argument("--loop-max", type=int, default=256)
    a = ap.parse_args()
    if a.projs + a.storage + a.scaling + a.slice_batch + a.compute + a.path_kernel + a.hoist + a.matrix + a.indirect + a.reuse + a.accumulate + a.resident + a.many + a.sample + a.sample_joint > 1:
        ap.error("--projs, --storage, --scaling, --slice-batch, --compute, --path-kernel, --hoist, --matrix, --indirect, --reuse, --accumulate, --resident, --many, --sample and --sample-joint each "
                 "append one leg: run them one after the other")
    lines = [f"# tools/time_contract.py on {torch.cuda.get_device_name(0)}; torch {torch.__version__}", ""]
    if a.projs or a.storage or a.scaling or a.slice_batch or a.compute or a.path_kernel or a.hoist or a.matrix or a.indirect or a.reuse or a.accumulate or a.resident or a.many or a.sample or a.sample_joint:  # (the other legs' sections stay as they are)
        if a.sample_joint:
            lines.append(f"(the leg below: {torch.cuda.get_device_name(0)}; torch {torch.__version__})")
            sample_joint(lines)
        elif a.sample:
            lines.append(f"(the leg below: {torch.cuda.get_device_name(0)}; torch {torch.__version__})")
            sample(lines)
        elif a.many:
            lines.append(f"(the leg below: {torch.cuda.get_device_name(0)}; torch {torch.__version__})")
            many(lines, a.depth, a.max_width, min(a.max_slices, 2048))
        elif a.resident:
            lines.append(f"(the leg below: {torch.cuda.get_device_name(0)}; torch {torch.__version__})")
            resident(lines, a.depth, a.max_width, min(a.max_slices, 2048))
        elif a.accumulate:
            lines.append(f"(the leg below: {torch.cuda.get_device_name(0)}; torch {torch.__version__})")
            accumulate(lines, a.depth, a.max_width, min(a.max_slices, 2048))
        elif a.reuse:
            lines.append(f"(the leg below: {torch.cuda.get_device_name(0)}; torch {torch.__version__})")
            reuse(lines, a.depth, a.max_width, min(a.max_slices, 2048))
        elif a.indirect:
            lines.append(f"(the leg below: {torch.cuda.get_device_name(0)}; torch {torch.__version__})")
            indirect(lines, a.depth, a.max_width, min(a.max_slices, 2048))
        elif a.matrix:
            lines.append(f"(the leg below: {torch.cuda.get_device_name(0)}; torch {torch.__version__})")
            matrix(lines, a.n)
        elif a.hoist:
            lines.append(f"(the leg below: {torch.cuda.get_device_name(0)}; torch {torch.__version__})")
            hoist(lines, a.depth, a.max_width, min(a.max_slices, 2048))
        elif a.path_kernel:
            lines.append(f"(the leg below: {torch.cuda.get_device_name(0)}; torch {torch.__version__})")
            path_kernel(lines, a.depth, a.max_width, min(a.max_slices, 2048))
        elif a.compute:
            lines.append(f"(the leg below: {torch.cuda.get_device_name(0)}; torch {torch.__version__})")
            compute(lines, a.n, a.depth, a.max_width, a.max_slices)
        elif a.slice_batch:
            slice_batch(lines, a.depth, a.max_width, min(a.max_slices, 2048))
        elif a.scaling:
            scaling(lines, a.n, a.depth, a.max_width, a.max_slices)
        elif a.storage:
            storage(lines, a.n, a.depth, a.max_width, a.max_slices)
        else:
            projections(lines, a.depth, a.counts, a.loop_max)
        with open(a.out, "a") as f:
            f.write("\n".join(lines[1:]) + "\n")
        return
    square(lines, a.n)
    skinny(lines)
    sycamore(lines, a.depth, a.max_width, a.max_slices)
    projections(lines, a.depth, a.counts, a.loop_max)
    storage(lines, a.n, a.depth, a.max_width, a.max_slices)
    scaling(lines, a.n, a.depth, a.max_width, a.max_slices)
    slice_batch(lines, a.depth, a.max_width, min(a.max_slices, 2048))
    compute(lines, a.n, a.depth, a.max_width, a.max_slices)
    path_kernel(lines, a.depth, a.max_width, min(a.max_slices, 2048))
    hoist(lines, a.depth, a.max_width, min(a.max_slices, 2048))
    matrix(lines, a.n)
    indirect(lines, a.depth, a.max_width, min(a.max_slices, 2048))
    reuse(lines, a.depth, a.max_width, min(a.max_slices, 2048))
    accumulate(lines, a.depth, a.max_width, min(a.max_slices, 2048))
    resident(lines, a.depth, a.max_width, min(a.max_slices, 2048))
    many(lines, a.depth, a.max_width, min(a.max_slices, 2048))
    sample(lines)
    sample_joint(lines)
    Path(a.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
