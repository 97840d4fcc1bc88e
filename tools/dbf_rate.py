"""
Pass times of the distance-to-boundary field and the segment table (run on the MI355X box):
    python tools/dbf_rate.py [--size 512] [--reps 5] [--worst-size 256] [--host-budget-s 240] [--out FILE]

Labels: inference.agglomerate_affinities(fragments="watershed", premerge_size=100,
return_device_tensor=True) on the neurite-like size^3 affinities of tools/watershed_rate.py. With HIP
events, the median of --reps runs after one warm-up of each leg, all on the same tensors in one run:
  x, y, z   the three passes of exaspim_dbf one by one, through the layer probe's probe_dbf_pass
            (launch_dbf_pass, the launcher exaspim_dbf itself calls three times), black_border = 0;
  dbf       exaspim_dbf, the three passes in one call;
  table     exaspim_segment_table with the field (its three launches; the one pass over the volume is
            all but a few microseconds of it).
The floor of a DBF pass is 12 bytes per voxel (labels and field read, field written), of the table
pass 8; each leg reports its bytes over its time as a fraction of 8 TB/s. The window depth of the y and
z passes is sqrt(result) probes per voxel: the mean over the foreground is reported with the times.
Worst case: one label filling --worst-size^3 with black_border = 0, where every field value stays
DBF_INF and the y and z passes walk every run to its end.
Host comparator: tests/dbf_ref.py per_label -- a per-label scipy EDT read through its indices, NOT the
edt package -- on the same labels on this host, wall time; past --host-budget-s it stops after the
label it is in and says how many labels and voxels it covered.
Writes the text report to --out (default profiles/dbf_pass_times_<size>.txt) and prints it.
"""

import argparse
import ctypes
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

HBM_BYTES_PER_S = 8e12


class _OverBudget(Exception):
    pass


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--worst-size", type=int, default=256)
    ap.add_argument("--host-budget-s", type=float, default=240.0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import numpy as np
    import torch

    import dbf_ref
    from aind_exaspim_neuron_segmentation_amd import _native, inference
    from aind_exaspim_neuron_segmentation_amd.utils import synthetic

    dev = torch.device("cuda:0")
    lib = _native.lib()
    probe = ctypes.CDLL(os.path.join(os.path.dirname(_native.LIB_PATH), "libexaspim_layer_probe.so"))
    probe.probe_dbf_pass.restype = ctypes.c_int
    probe.probe_dbf_pass.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                     ctypes.c_int32 * 3, ctypes.c_int, ctypes.c_void_p]
    lines = []

    def say(text=""):
        print(text, flush=True)
        lines.append(text)

    def neurite_affinities(n):
        gen = torch.Generator(device=dev)
        gen.manual_seed(5)
        raw = torch.empty((n, n, n), dtype=torch.int16, device=dev)
        _native.check(lib.exaspim_synth_volume_neurite_u16(raw.data_ptr(), _native.Block.make((n, n, n)), 0, None),
                      "synth_neurite")
        on = ((raw.to(torch.int32) & 0xFFFF) > synthetic.NEURITE_FLOOR_MAX).float()
        del raw
        p = torch.nn.functional.avg_pool3d(on[None, None], 3, stride=1, padding=1, count_include_pad=True)[0, 0]
        del on
        aff = torch.rand((3, n, n, n), dtype=torch.float32, device=dev, generator=gen).mul_(0.6).add_(0.4)
        aff[0, :-1] *= torch.minimum(p[:-1], p[1:])
        aff[1, :, :-1] *= torch.minimum(p[:, :-1], p[:, 1:])
        aff[2, :, :, :-1] *= torch.minimum(p[:, :, :-1], p[:, :, 1:])
        return aff

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    def median_ms(fn):
        timed(fn)      # warm-up
        return statistics.median(timed(fn) for _ in range(args.reps))

    def measure(title, labels, k):
        """The legs on one label tensor; returns the field."""
        shape = tuple(labels.shape)
        vox = float(labels.numel())
        dims = _native.int3(shape)
        field = torch.empty(shape, dtype=torch.int32, device=dev)
        mid = torch.empty(shape, dtype=torch.int32, device=dev)
        need = lib.exaspim_dbf_workspace_bytes(dims)
        ws = torch.empty(need, dtype=torch.uint8, device=dev)

        def one_pass(axis, src, dst):
            def call():
                _native.check(probe.probe_dbf_pass(axis, labels.data_ptr(), src.data_ptr() if src is not None else None,
                                                   dst.data_ptr(), dims, 0, None), "probe_dbf_pass")
            return call

        def whole():
            _native.check(lib.exaspim_dbf(labels.data_ptr(), dims, 0, field.data_ptr(), ws.data_ptr(), need, None),
                          "exaspim_dbf")

        say(f"{title}: {shape[0]} x {shape[1]} x {shape[2]}, {k} labels, "
            f"{float((labels > 0).sum()) / vox:.4f} of the voxels foreground")
        legs = [("x", one_pass(2, None, field), 12), ("y", one_pass(1, field, mid), 12),
                ("z", one_pass(0, mid, field), 12), ("dbf", whole, 36)]
        for name, fn, bytes_per_voxel in legs:      # in this order: each pass reads what the one before left
            ms = median_ms(fn)
            say(f"  {name:<6}{ms:10.3f} ms  {vox / (ms * 1e-3):.3e} voxels/s  "
                f"{bytes_per_voxel * vox / (ms * 1e-3) / HBM_BYTES_PER_S:6.3f} of 8 TB/s at {bytes_per_voxel} B/voxel")
        tneed = lib.exaspim_segment_table_workspace_bytes(k)
        outs = [torch.empty(k + 1, dtype=torch.int64, device=dev), torch.empty((k + 1, 6), dtype=torch.int32, device=dev),
                torch.empty(k + 1, dtype=torch.int32, device=dev), torch.empty(k + 1, dtype=torch.int32, device=dev)]
        tws = torch.empty(tneed, dtype=torch.uint8, device=dev)

        def table():
            _native.check(lib.exaspim_segment_table(labels.data_ptr(), field.data_ptr(), dims, k,
                                                    *[t.data_ptr() for t in outs], tws.data_ptr(), tneed, None),
                          "exaspim_segment_table")

        ms = median_ms(table)
        say(f"  {'table':<6}{ms:10.3f} ms  {vox / (ms * 1e-3):.3e} voxels/s  "
            f"{8 * vox / (ms * 1e-3) / HBM_BYTES_PER_S:6.3f} of 8 TB/s at 8 B/voxel")
        finite = field[(labels > 0) & (field != inference.DBF_INF)].double()
        if finite.numel():
            say(f"  window depth sqrt(dbf) over the foreground with a finite field: mean {float(finite.sqrt().mean()):.2f}, "
                f"largest {float(finite.max()) ** 0.5:.2f}; largest peak {int(outs[2].max())}")
        else:
            say("  every foreground voxel is DBF_INF: the y and z passes walk whole runs")
        return field

    n = args.size
    say(f"tools/dbf_rate.py --size {n} --reps {args.reps} --worst-size {args.worst_size} on {torch.cuda.get_device_name(0)}: "
        f"HIP events, median of {args.reps} after a warm-up")
    aff = neurite_affinities(n)
    # twice the watershed's contacts on this tensor, the next power of two (tools/watershed_rate.py sizes it by a run:
    # 5.7e6 edges at 512^3)
    capacity = max(1 << 16, 1 << (n ** 3 // 8 - 1).bit_length())
    labels = inference.agglomerate_affinities(aff, fragments="watershed", premerge_size=100, edge_capacity=capacity,
                                              return_device_tensor=True)
    del aff
    torch.cuda.empty_cache()
    k = int(labels.max())
    field = measure("neurite-like", labels, k)

    host = labels.cpu().numpy()
    got = field.cpu().numpy()
    del labels, field
    torch.cuda.empty_cache()
    worst = torch.full((args.worst_size,) * 3, 1, dtype=torch.int32, device=dev)
    measure("worst case, one label everywhere, black_border = 0", worst, 1)
    del worst

    t0 = time.perf_counter()
    done = [0, 0]

    def on_label(rank, total):
        done[:] = [rank, total]
        print(f"host oracle: label {rank} of {total}, {time.perf_counter() - t0:.1f} s", file=sys.stderr, flush=True)
        if time.perf_counter() - t0 > args.host_budget_s:
            raise _OverBudget()

    try:
        want = dbf_ref.per_label(host, False, on_label=on_label)
        wall = time.perf_counter() - t0
        same = bool(np.array_equal(want, got))
        say(f"host comparator, tests/dbf_ref.py per_label (a per-label scipy EDT, not edt) on the same labels: "
            f"{wall:.1f} s wall; its field equals the device's: {same}")
    except _OverBudget:
        wall = time.perf_counter() - t0
        say(f"host comparator, tests/dbf_ref.py per_label (a per-label scipy EDT, not edt) on the same labels: stopped "
            f"at --host-budget-s after {done[0]} of {done[1]} labels in {wall:.1f} s wall")

    out = args.out or os.path.join(ROOT, "profiles", f"dbf_pass_times_{n}.txt")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
