"""
What the region graph of a volume costs slab by slab over the whole-volume call (run on the
MI355X box):
    python tools/region_graph_stream_rate.py [--size 512] [--slab 64] [--reps 5] [--predict] [--out FILE]

On one size^3 float32 volume per case that still fits the device, with HIP events, the median of --reps
runs after one warm-up of each leg, the legs alternating in one run on the same tensors (the two tensors
of tools/region_graph_rate.py: neurite-like dimmed affinities at fragment threshold 0.5, uniform random
affinities at 0.75):
  whole     exaspim_region_graph on the final fragments (exaspim_components, min_size 0) and the whole
            tensor: memsets, the tile pass, the compaction; no download;
  streamed  the sum of its two parts, timed in the same run --
  slabs     exaspim_region_graph_stream_slab for every z slab of --slab planes, on the provisional ids a
            ComponentsStream(min_segment_size=0) wrote for the same slabs beforehand (labelling is not part
            of either leg): the reset, per slab the seam pass, the tile pass and the carry pass,
  finish    exaspim_region_graph_stream_finish with ComponentsStream's table: the retarget pass, the sizes
            pass, the compaction; no download.
Both legs use one edge_capacity: the power of two above twice the PROVISIONAL keys, which a first run
with room for every edge counts. The two edge lists are compared on the device after sorting.
--predict adds, host array to host array with the default model (fp16, batch 16), one warm-up and one
timed run each:
  predict_components_streaming   threshold 0.5, min size 0: the fragments;
  predict_agglomerate_streaming  the same fragments, their graph, the merge on the host, the composed table.
The second is skipped, and the JSON says so, when there are more than --max-fragments fragments: merging
the graph of ten million fragments on the host takes minutes.
Prints one JSON line; --out also writes it to a file, after every case.
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--slab", type=int, default=64)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cases", default="neurite,random")
    ap.add_argument("--predict", action="store_true")
    ap.add_argument("--max-fragments", type=int, default=2_000_000)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import numpy as np
    import torch

    from aind_exaspim_neuron_segmentation_amd import _native, inference
    from aind_exaspim_neuron_segmentation_amd.utils import synthetic

    dev = torch.device("cuda:0")
    n = args.size
    vox = float(n) ** 3
    lib = _native.lib()
    dims = _native.int3((n, n, n))
    gen = torch.Generator(device=dev)
    gen.manual_seed(5)

    def neurite():
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

    def random():
        return torch.rand((3, n, n, n), dtype=torch.float32, device=dev, generator=gen)

    def event():
        e = torch.cuda.Event(enable_timing=True)
        e.record()
        return e

    def log(*what):
        print(*what, file=sys.stderr, flush=True)

    def write(res):
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                f.write(json.dumps(res) + "\n")

    def sorted_graph(edges, counts, sums, n_edges):
        key = (edges[:n_edges, 0].long() << 32) | edges[:n_edges, 1].long()
        order = torch.argsort(key)
        return key[order], counts[:n_edges][order], sums[:n_edges][order]

    parts = [(z0, min(z0 + args.slab, n)) for z0 in range(0, n, args.slab)]
    cases = {"neurite": (neurite, 0.5), "random": (random, 0.75)}
    res = {"size": n, "slab_depth": args.slab, "reps": args.reps, "device": torch.cuda.get_device_name(0),
           "cases": {}}
    for kind in [c for c in args.cases.split(",") if c]:
        make, fragment_threshold = cases[kind]
        aff = make()
        # slabs are contiguous (3, d, H, W) tensors when they arrive; cutting them out of the whole tensor
        # is not part of the graph
        slabs = [aff[:, z0:z1].contiguous() for z0, z1 in parts]
        fragments, count = inference._components_on_device(aff, fragment_threshold, 0)
        k = int(count.cpu()[0])
        cs = inference.ComponentsStream((n, n, n), fragment_threshold, 0, device=dev, id_capacity=min(n ** 3, 1 << 27))
        provisional = torch.empty((n, n, n), dtype=torch.int32, device=dev)
        for (z0, z1), slab in zip(parts, slabs):
            cs.push(slab, z0, provisional[z0:z1])
        table, k_streamed = cs.finish()
        table = table[: cs.ids_used + 1]
        assert k_streamed == k, (k_streamed, k)
        stream = torch.cuda.current_stream(dev).cuda_stream
        bufs = {}

        def allocate(capacity):
            bufs.clear()
            torch.cuda.empty_cache()
            need = max(lib.exaspim_region_graph_workspace_bytes(dims, k, capacity),
                       lib.exaspim_region_graph_stream_finish_workspace_bytes(capacity))
            for name in ("whole", "streamed"):
                bufs[name] = dict(edges=torch.empty((capacity, 2), dtype=torch.int32, device=dev),
                                  counts=torch.empty(capacity, dtype=torch.int64, device=dev),
                                  sums=torch.empty(capacity, dtype=torch.int64, device=dev),
                                  sizes=torch.empty(k + 1, dtype=torch.int64, device=dev),
                                  state=torch.empty(2, dtype=torch.int32, device=dev))
            bufs["ws"] = torch.empty(need, dtype=torch.uint8, device=dev)
            bufs["rgs"] = inference.RegionGraphStream((n, n, n), device=dev, id_capacity=cs.id_capacity,
                                                      edge_capacity=capacity)
            bufs["capacity"] = capacity

        def whole():
            b = bufs["whole"]
            a = event()
            _native.check(
                lib.exaspim_region_graph(fragments.data_ptr(), aff.data_ptr(), _native.AFF_F32, dims, k,
                                         bufs["capacity"], b["edges"].data_ptr(), b["counts"].data_ptr(),
                                         b["sums"].data_ptr(), b["sizes"].data_ptr(), b["state"].data_ptr(),
                                         bufs["ws"].data_ptr(), bufs["ws"].numel(), stream),
                "exaspim_region_graph")
            e = event()
            e.synchronize()
            return {"whole": a.elapsed_time(e)}

        def streamed():
            b, rgs = bufs["streamed"], bufs["rgs"]
            rgs.desc.next_z = 0
            a = event()
            for (z0, z1), slab in zip(parts, slabs):
                rgs.push(provisional[z0:z1], slab, z0)
            m = event()
            _native.check(
                lib.exaspim_region_graph_stream_finish(
                    ctypes.byref(rgs.desc), table.data_ptr(), table.numel(), k, b["edges"].data_ptr(),
                    b["counts"].data_ptr(), b["sums"].data_ptr(), b["sizes"].data_ptr(), b["state"].data_ptr(),
                    bufs["ws"].data_ptr(), bufs["ws"].numel(), stream),
                "exaspim_region_graph_stream_finish")
            e = event()
            e.synchronize()
            t = {"slabs": a.elapsed_time(m), "finish": m.elapsed_time(e)}
            t["streamed"] = t["slabs"] + t["finish"]
            return t

        # a first run with room for every edge the volume can have counts the provisional keys
        capacity = min(1 << 30, 1 << (3 * n ** 3 - 1).bit_length())
        while capacity > (1 << 16) and 5 * 24 * capacity > torch.cuda.mem_get_info(dev)[0] // 2:
            capacity >>= 1
        allocate(capacity)
        streamed()
        n_edges, overflow = (int(v) for v in bufs["streamed"]["state"].cpu())
        assert not overflow, (kind, capacity)
        provisional_keys = int((bufs["rgs"].keys != -1).sum())
        capacity = max(1 << 16, 1 << (2 * provisional_keys - 1).bit_length())
        allocate(capacity)
        log(f"{kind}: {k} fragments, {cs.ids_used} provisional ids, {provisional_keys} provisional keys, "
            f"{n_edges} edges, edge_capacity {capacity}")
        whole()
        streamed()      # the warm-up of each leg, and what is compared
        states = {name: [int(v) for v in bufs[name]["state"].cpu()] for name in ("whole", "streamed")}
        assert states["whole"] == states["streamed"] == [n_edges, 0], states
        w = sorted_graph(bufs["whole"]["edges"], bufs["whole"]["counts"], bufs["whole"]["sums"], n_edges)
        s = sorted_graph(bufs["streamed"]["edges"], bufs["streamed"]["counts"], bufs["streamed"]["sums"], n_edges)
        equal = all(torch.equal(x, y) for x, y in zip(w, s)) and torch.equal(bufs["whole"]["sizes"],
                                                                             bufs["streamed"]["sizes"])
        del w, s
        entry = {"fragment_threshold": fragment_threshold, "fragments": k, "provisional_ids": cs.ids_used,
                 "provisional_keys": provisional_keys, "edges": n_edges, "edge_capacity": capacity,
                 "slabs": len(parts), "equals_whole_volume": bool(equal)}
        times = {}
        for _ in range(args.reps):
            for t in (whole(), streamed()):
                for name, v in t.items():
                    times.setdefault(name, []).append(v)
        entry["legs"] = {name: {"median_ms": statistics.median(v), "ms": v} for name, v in times.items()}
        med = {name: v["median_ms"] for name, v in entry["legs"].items()}
        entry["streamed_over_whole"] = med["streamed"] / med["whole"]
        entry["slabs_over_whole"] = med["slabs"] / med["whole"]
        entry["voxels_per_s_streamed"] = vox / (med["streamed"] * 1e-3)
        log(f"{kind}: " + ", ".join(f"{name} {v:.2f} ms" for name, v in med.items()))
        res["cases"][kind] = entry
        del aff, slabs, fragments, provisional, table, cs
        bufs.clear()
        torch.cuda.empty_cache()
        write(res)

    if args.predict:
        from aind_exaspim_neuron_segmentation_amd.machine_learning.unet3d import UNet3D

        sd = synthetic.synth_state_dict(3, 1, seed=1)
        model = UNet3D(output_channels=3, compute_dtype="fp16")
        model.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in sd.items()})
        model.to(dev).eval()
        raw = torch.empty((n, n, n), dtype=torch.int16, device=dev)
        _native.check(lib.exaspim_synth_volume_neurite_u16(raw.data_ptr(), _native.Block.make((n, n, n)), 0, None),
                      "synth_neurite")
        vol = raw.cpu().numpy().view(np.uint16)
        del raw
        pred = {"runs": "one warm-up and one timed run of each leg"}

        def leg(name, fn):
            fn({})
            timings = {}
            t0 = time.perf_counter()
            out = fn(timings)
            pred[name] = {"seconds": time.perf_counter() - t0, "timings": timings, "dtype": str(out.dtype),
                          "bytes": int(out.nbytes), "labels": int(out.max())}
            log(f"{name}: {pred[name]['seconds']:.2f} s, {pred[name]['labels']} labels")
            write(dict(res, predict=pred))

        # room for the ids and keys of shallow noisy slabs: the defaults suit a real volume's fragments
        ids, slots = min(n ** 3, 1 << 26), 1 << 26
        pred["id_capacity"], pred["edge_capacity"] = ids, slots
        leg("predict_components_streaming",
            lambda t: inference.predict_components_streaming(vol, model, 0.5, 0, verbose=False, timings=t,
                                                             id_capacity=ids))
        fragments = pred["predict_components_streaming"]["labels"]
        if fragments > args.max_fragments:
            pred["predict_agglomerate_streaming"] = {
                "skipped": f"{fragments} fragments, more than --max-fragments {args.max_fragments}: the host merge "
                           "would take minutes"}
        else:
            leg("predict_agglomerate_streaming",
                lambda t: inference.predict_agglomerate_streaming(vol, model, verbose=False, timings=t,
                                                                  id_capacity=ids, edge_capacity=slots))
            pred["agglomerate_over_components"] = (pred["predict_agglomerate_streaming"]["seconds"]
                                                   / pred["predict_components_streaming"]["seconds"])
        res["predict"] = pred
        write(res)

    print(json.dumps(res))
    if not all(c["equals_whole_volume"] for c in res["cases"].values()):
        sys.exit(1)


if __name__ == "__main__":
    main()
