"""
Pass times of fill_holes (run on the MI355X box):
    python tools/holes_rate.py [--size 512] [--reps 5] [--host-budget-s 240] [--out FILE]

Labels: those of tools/dbf_rate.py -- inference.agglomerate_affinities(fragments="watershed",
premerge_size=100, return_device_tensor=True) on the neurite-like size^3 affinities. Two legs on them:
  as_is    the labels as they are;
  punched  the same labels with every 97th interior foreground voxel (one whose six neighbours carry its
           own label) set to 0 in raster order, so that holes exist.
Per leg, with HIP events, the median of --reps runs after one warm-up: exaspim_fill_holes as one call, and
its six passes one by one through the layer probe's probe_fill_holes_passes (launch_fill_holes_passes, the
launcher exaspim_fill_holes itself runs from end to end), each on what the ones before left in the
workspace (the parent array written afresh, untimed, before every run of a pass that changes it); the two
counts; the wall time of tests/holes_ref.py per_label (a per-label scipy binary_fill_holes inside each
label's bounding box) on the same labels on this host, and whether the device's labels equal it. Past
--host-budget-s the oracle stops after the label it is in and says so. The byte floor of the passes is
about 40 bytes per voxel; each leg reports it over its time as a fraction of 8 TB/s. Writes one JSON
document to --out (default profiles/holes_rate_<size>.json) and prints it.
"""

import argparse
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

HBM_BYTES_PER_S = 8e12
PASSES = ["edge_mask_background", "tile_pass", "face_merge", "flatten", "survey", "fill"]
# bytes per voxel each pass has to move at least: labels in and mask out; mask in and parent out; mask in;
# parent in; the two words reset, mask and parent in; labels and parent in, labels out
FLOOR = [5, 5, 1, 4, 13, 12]


class _OverBudget(Exception):
    pass


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-budget-s", type=float, default=240.0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import numpy as np
    import torch

    import holes_ref
    from aind_exaspim_neuron_segmentation_amd import _native, inference
    from aind_exaspim_neuron_segmentation_amd.utils import synthetic

    dev = torch.device("cuda:0")
    lib = _native.lib()
    probe = ctypes.CDLL(os.path.join(os.path.dirname(_native.LIB_PATH), "libexaspim_layer_probe.so"))
    probe.probe_fill_holes_passes.restype = ctypes.c_int
    probe.probe_fill_holes_passes.argtypes = [ctypes.c_void_p, ctypes.c_int32 * 3, ctypes.c_void_p, ctypes.c_void_p,
                                              ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]

    def neurite_affinities(n):      # the tensor of tools/dbf_rate.py
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

    def timed(fn, before=None):
        if before is not None:
            before()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    def median_ms(fn, before=None):
        timed(fn, before)      # warm-up
        return statistics.median(timed(fn, before) for _ in range(args.reps))

    def punch(labels):
        """Every 97th interior foreground voxel, in raster order, set to 0 in a copy."""
        interior = labels > 0
        interior[0] = interior[-1] = False
        interior[:, 0] = interior[:, -1] = False
        interior[:, :, 0] = interior[:, :, -1] = False
        interior[1:-1] &= (labels[1:-1] == labels[2:]) & (labels[1:-1] == labels[:-2])
        interior[:, 1:-1] &= (labels[:, 1:-1] == labels[:, 2:]) & (labels[:, 1:-1] == labels[:, :-2])
        interior[:, :, 1:-1] &= (labels[:, :, 1:-1] == labels[:, :, 2:]) & (labels[:, :, 1:-1] == labels[:, :, :-2])
        chosen = interior.reshape(-1).nonzero().reshape(-1)[::97]
        out = labels.clone()
        out.reshape(-1)[chosen] = 0
        return out, int(interior.sum()), int(chosen.numel())

    def measure(name, labels):
        shape = tuple(labels.shape)
        vox = float(labels.numel())
        dims = _native.int3(shape)
        need = lib.exaspim_fill_holes_workspace_bytes(dims)
        out = torch.empty(shape, dtype=torch.int32, device=dev)
        counts = torch.empty(2, dtype=torch.int64, device=dev)
        ws = torch.empty(need, dtype=torch.uint8, device=dev)

        def whole():
            _native.check(lib.exaspim_fill_holes(labels.data_ptr(), dims, out.data_ptr(), counts.data_ptr(),
                                                 ws.data_ptr(), need, None), "exaspim_fill_holes")

        def passes(first, last):
            def call():
                _native.check(probe.probe_fill_holes_passes(labels.data_ptr(), dims, out.data_ptr(), counts.data_ptr(),
                                                            ws.data_ptr(), first, last, None),
                              "probe_fill_holes_passes")
            return call

        leg = {"leg": name, "shape": list(shape), "labels": int(labels.max()),
               "foreground_fraction": float((labels > 0).sum()) / vox, "workspace_bytes": int(need)}
        ms = median_ms(whole)
        leg["fill_holes_ms"] = ms
        leg["voxels_per_s"] = vox / (ms * 1e-3)
        leg["fraction_of_8TBps_at_40B_per_voxel"] = 40 * vox / (ms * 1e-3) / HBM_BYTES_PER_S
        leg["pass_ms"] = {}
        for k, title in enumerate(PASSES):      # in this order: each pass reads what the one before left
            # face_merge and flatten change the parent array they read: tile_pass writes it afresh, untimed,
            # before every run of theirs
            leg["pass_ms"][title] = median_ms(passes(k, k), passes(1, k - 1) if k in (2, 3) else None)
        leg["pass_floor_bytes_per_voxel"] = dict(zip(PASSES, FLOOR))
        whole()
        torch.cuda.synchronize()
        leg["holes_filled"], leg["voxels_filled"] = (int(v) for v in counts.cpu())
        got = out.cpu().numpy()
        host = labels.cpu().numpy()
        del out, ws
        torch.cuda.empty_cache()

        t0 = time.perf_counter()
        done = [0, 0]

        def on_label(rank, total):
            done[:] = [rank, total]
            print(f"host oracle ({name}): label {rank} of {total}, {time.perf_counter() - t0:.1f} s", file=sys.stderr,
                  flush=True)
            if time.perf_counter() - t0 > args.host_budget_s:
                raise _OverBudget()

        try:
            want, enclosed = holes_ref.per_label(host, on_label=on_label)
            leg["host_per_label_s"] = time.perf_counter() - t0
            leg["host_reports_an_enclosed_label"] = bool(enclosed)
            leg["device_equals_host_per_label"] = bool(np.array_equal(want, got))
        except _OverBudget:
            leg["host_per_label_s"] = time.perf_counter() - t0
            leg["host_stopped_after_labels"] = done
        print(json.dumps(leg), flush=True)
        return leg

    n = args.size
    report = {"tool": f"tools/holes_rate.py --size {n} --reps {args.reps}", "device": torch.cuda.get_device_name(0),
              "timing": f"HIP events, median of {args.reps} after a warm-up", "legs": []}
    aff = neurite_affinities(n)
    capacity = max(1 << 16, 1 << (n ** 3 // 8 - 1).bit_length())      # as tools/dbf_rate.py sizes it
    labels = inference.agglomerate_affinities(aff, fragments="watershed", premerge_size=100, edge_capacity=capacity,
                                              return_device_tensor=True)
    del aff
    torch.cuda.empty_cache()
    report["legs"].append(measure("as_is", labels))
    punched, interior, chosen = punch(labels)
    del labels
    torch.cuda.empty_cache()
    leg = measure("punched", punched)
    leg["interior_foreground_voxels"], leg["voxels_set_to_0"] = interior, chosen
    report["legs"].append(leg)

    out = args.out or os.path.join(ROOT, "profiles", f"holes_rate_{n}.json")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(report, f, indent=1)
        f.write("\n")
    print(json.dumps(report, indent=1))


if __name__ == "__main__":
    main()
