"""
Rate of the mean-affinity agglomeration (run on the MI355X box):
    python tools/region_graph_rate.py [--size 512] [--reps 5] [--slow-s 20] [--out FILE]

On one size^3 float32 volume per case, with HIP events, the median of --reps runs after one warm-up of
each leg, all legs of a case on the same tensors in the same run:
  components    exaspim_components at the fragment threshold, min_size 0 (the fragments);
  region_graph  exaspim_region_graph on those fragments and the same affinities (the ABI call alone:
                memsets, the tile pass, the compaction; no download);
  whole         inference.agglomerate_affinities(..., return_device_tensor=True): fragments, region
                graph, the download of E x 24 B + K x 8 B, the sort, exaspim_agglomerate on the host, the
                table's upload and apply_table. Its host part is timed separately (host_ms);
  download      what the feature replaces: .cpu() of the same 12-byte-per-voxel tensor;
  labels        .cpu() of the 4-byte-per-voxel int32 labels that leave the device instead.
A leg whose warm-up takes longer than --slow-s seconds is not repeated: its one run is what is reported
(reps_used 1).
Cases:
  neurite   the neurite-like volume (exaspim_synth_volume_neurite_u16 > NEURITE_FLOOR_MAX), its mask
            smoothed with a 3^3 box so that values fall off across a tube's wall, and every edge dimmed by
            its own uniform factor in [0.4, 1]: aff_c[v] = min(p[v], p[v + e_c]) * (0.4 + 0.6 u_c[v]). Tubes
            break into fragments at dim edges and the contacts have means anywhere in 0 .. 0.5: not binary.
            Fragment threshold 0.5, agglomeration thresholds 0.6, 0.8, 0.9, min_segment_size 100;
  random    uniform random affinities at fragment threshold 0.75, at the bond percolation threshold of the
            cubic lattice: the adversarial case (a fragment per ten voxels, a distinct contact per two).
Prints one JSON line; --out also writes it to a file.
"""

import argparse
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
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--slow-s", type=float, default=20.0)
    ap.add_argument("--cases", default="neurite,random")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch

    from aind_exaspim_neuron_segmentation_amd import _native, inference
    # agglomerate_affinities resolves agglomerate in segmentation's globals: that is the name to rebind
    from aind_exaspim_neuron_segmentation_amd import segmentation as seg_module
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

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b), out

    def log(*what):
        print(*what, file=sys.stderr, flush=True)

    cases = {"neurite": (neurite, 0.5), "random": (random, 0.75)}
    thresholds, min_size = [0.6, 0.8, 0.9], 100
    res = {"size": n, "reps": args.reps, "device": torch.cuda.get_device_name(0), "thresholds": thresholds,
           "min_segment_size": min_size, "cases": {}}
    for kind in args.cases.split(","):
        make, fragment_threshold = cases[kind]
        aff = make()
        torch.cuda.synchronize()
        labels, count = inference._components_on_device(aff, fragment_threshold, 0)
        k = int(count.cpu()[0])
        # the table: a first run with room for every edge the volume can have, then twice the edges it found,
        # so that the load stays under a half
        capacity = min(1 << 30, 1 << (3 * n ** 3 - 1).bit_length())
        while capacity > (1 << 16) and lib.exaspim_region_graph_workspace_bytes(dims, k, capacity) * 2 > \
                torch.cuda.mem_get_info(dev)[0] // 2:
            capacity >>= 1
        bufs = {}

        def graph_call():
            _native.check(
                lib.exaspim_region_graph(labels.data_ptr(), aff.data_ptr(), _native.AFF_F32, dims, k, capacity,
                                         bufs["edges"].data_ptr(), bufs["counts"].data_ptr(), bufs["sums"].data_ptr(),
                                         bufs["sizes"].data_ptr(), bufs["state"].data_ptr(), bufs["ws"].data_ptr(),
                                         bufs["ws"].numel(), torch.cuda.current_stream(dev).cuda_stream),
                "exaspim_region_graph")

        def allocate():
            bufs.clear()
            torch.cuda.empty_cache()
            bufs.update(
                edges=torch.empty((capacity, 2), dtype=torch.int32, device=dev),
                counts=torch.empty(capacity, dtype=torch.int64, device=dev),
                sums=torch.empty(capacity, dtype=torch.int64, device=dev),
                sizes=torch.empty(k + 1, dtype=torch.int64, device=dev),
                state=torch.empty(2, dtype=torch.int32, device=dev),
                ws=torch.empty(lib.exaspim_region_graph_workspace_bytes(dims, k, capacity), dtype=torch.uint8,
                               device=dev))

        allocate()
        graph_call()
        n_edges, overflow = (int(v) for v in bufs["state"].cpu())
        assert not overflow, (kind, capacity)
        capacity = max(1 << 16, 1 << (2 * n_edges - 1).bit_length())
        allocate()
        log(f"{kind}: {k} fragments, {n_edges} edges, edge_capacity {capacity}")

        host = []

        def whole():
            real = seg_module.agglomerate

            def clocked(*a, **kw):
                t0 = time.perf_counter()
                out = real(*a, **kw)
                host.append((time.perf_counter() - t0) * 1e3)
                return out

            seg_module.agglomerate = clocked
            try:
                return inference.agglomerate_affinities(aff, thresholds, min_size,
                                                        fragment_threshold=fragment_threshold,
                                                        edge_capacity=capacity, return_device_tensor=True)
            finally:
                seg_module.agglomerate = real

        legs = {
            "components": lambda: inference._components_on_device(aff, fragment_threshold, 0),
            "region_graph": graph_call,
            "whole": whole,
            "download": lambda: aff.cpu(),
        }
        entry = {"fragment_threshold": fragment_threshold, "fragments": k, "edges": n_edges,
                 "edge_capacity": capacity, "legs": {}}
        reps = {}
        segmentation = None
        for name, fn in legs.items():      # warm-up
            ms, out = timed(fn)
            reps[name] = 1 if ms > args.slow_s * 1e3 else args.reps
            entry["legs"][name] = {"warmup_ms": ms}
            if name == "whole":
                segmentation = out
                entry["segments"] = int(out.max())
                entry["legs"][name]["warmup_host_ms"] = host[-1]
            del out
            log(f"{kind}: warm-up of {name} {ms:.1f} ms")
        legs["labels"] = lambda: segmentation.cpu()
        reps["labels"] = args.reps
        entry["legs"]["labels"] = {"warmup_ms": timed(legs["labels"])[0]}
        host.clear()
        for name, fn in legs.items():
            leg = entry["legs"][name]
            if reps[name] == 1 and name != "labels":
                ts = [leg["warmup_ms"]]
                if name == "whole":
                    leg["host_ms"] = leg["warmup_host_ms"]
            else:
                ts = []
                for _ in range(reps[name]):
                    ms, out = timed(fn)
                    del out
                    ts.append(ms)
                if name == "whole":
                    leg["host_ms"] = statistics.median(host)
            med = statistics.median(ts)
            leg.update({"median_ms": med, "ms": ts, "reps_used": len(ts), "voxels_per_s": vox / (med * 1e-3)})
            log(f"{kind}: {name} median {med:.2f} ms of {len(ts)}")
        med = {name: leg["median_ms"] for name, leg in entry["legs"].items()}
        entry["whole_plus_labels_ms"] = med["whole"] + med["labels"]
        entry["beats_download"] = entry["whole_plus_labels_ms"] < med["download"]
        res["cases"][kind] = entry
        del aff, labels, segmentation
        bufs.clear()
        torch.cuda.empty_cache()
        if args.out:      # after every case: a later one may be cut short
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                f.write(json.dumps(res) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
