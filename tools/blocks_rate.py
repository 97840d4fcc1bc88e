"""
skeletonize_blocks next to skeletonize_pieces on the device (run on the MI355X box):
    python tools/blocks_rate.py [--size 512] [--reps 5] [--out FILE]

Labels as in tools/pieces_rate.py: the neurite-like size^3 affinities,
agglomerate_affinities(fragments="watershed", premerge_size=100), fill_holes. Recorded, all in the same run:
  label_pieces_open   exaspim_label_pieces_open through the C ABI into buffers made once, with no face open and with
                      all six, at dust 1000, with the three state words;
  mark_pass_ms        the difference of the two: the launches are otherwise the same. The C ABI has one entry for
                      all launches, so the new pass itself and its yardstick, pieces_sizes on the same tensor, are
                      timed with a kernel trace of
                          rocprofv3 --kernel-trace --stats -- python tools/blocks_rate.py --kernels-only
                      (1 + --reps calls of each form and nothing else of what follows);
  skeletonize_blocks  the whole call on the device tensor with block_shape (size / 2 + 1)^3, eight blocks, the
                      reference's teasar_params: milliseconds, and the trees, joints and skipped joints;
  skeletonize_pieces  the whole call on the whole tensor: milliseconds and trees.
HIP events, the median of --reps runs after one warm-up. Nothing here is a pass criterion: whether eight blocks with
fewer given rounds each are faster or slower than one is what this run finds out. Writes one JSON object to --out
(default profiles/skeletonize_blocks_<size>.json) and prints it.
"""

import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--kernels-only", action="store_true",
                    help="only the C-ABI calls, for a kernel trace: no skeletons, no file")
    args = ap.parse_args()

    import torch

    from aind_exaspim_neuron_segmentation_amd import _native, inference
    from aind_exaspim_neuron_segmentation_amd.utils import synthetic

    dev = torch.device("cuda:0")
    lib = _native.lib()

    def neurite_affinities(n):      # tools/geodesic_rate.py's
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
        return round(statistics.median(timed(fn) for _ in range(args.reps)), 3)

    n = args.size
    aff = neurite_affinities(n)
    capacity = max(1 << 16, 1 << (n ** 3 // 8 - 1).bit_length())
    labels = inference.agglomerate_affinities(aff, fragments="watershed", premerge_size=100, edge_capacity=capacity,
                                              return_device_tensor=True)
    del aff
    labels, _ = inference._fill_holes_on_device(labels)
    torch.cuda.empty_cache()
    k = max(int(labels.max()), 0)
    shape = tuple(labels.shape)
    dims = _native.int3(shape)
    report = {
        "tool": f"tools/blocks_rate.py --size {n} --reps {args.reps}",
        "device": torch.cuda.get_device_name(0), "shape": list(shape), "labels": k,
        "foreground_voxels": int((labels > 0).sum()),
        "timing": f"HIP events, median of {args.reps} after a warm-up",
    }

    need = lib.exaspim_label_pieces_open_workspace_bytes(dims)
    pieces = torch.empty(shape, dtype=torch.int32, device=dev)
    state = torch.empty(3, dtype=torch.int32, device=dev)
    workspace = torch.empty(need, dtype=torch.uint8, device=dev)
    calls = {}
    for name, mask in (("no_face_open", 0), ("six_faces_open", 63)):
        def kernels():
            _native.check(lib.exaspim_label_pieces_open(labels.data_ptr(), dims, k, 1000, mask, pieces.data_ptr(),
                                                        state.data_ptr(), workspace.data_ptr(), need, None),
                          "label_pieces_open")

        calls[name] = {"label_pieces_open_kernels_ms": median_ms(kernels)}
        calls[name]["pieces"], calls[name]["dust_pieces"], calls[name]["open_small_pieces"] = (
            int(v) for v in state.cpu())
        print(json.dumps({name: calls[name]}), flush=True)
    report["label_pieces_open"] = calls
    report["mark_pass_ms"] = round(calls["six_faces_open"]["label_pieces_open_kernels_ms"]
                                   - calls["no_face_open"]["label_pieces_open_kernels_ms"], 3)
    report["face_pixels"] = 6 * n * n
    if args.kernels_only:
        return
    del pieces, workspace
    torch.cuda.empty_cache()

    block = n // 2 + 1
    stats, forests = {}, {}
    report["skeletonize_blocks"] = {
        "block_shape": [block] * 3,
        "ms": median_ms(lambda: forests.update(inference.skeletonize_blocks(labels, (block,) * 3, stats=stats))),
    }
    report["skeletonize_blocks"].update(
        {key: (round(stats[key], 3) if key.endswith("seconds") else stats[key]) for key in sorted(stats)})
    report["skeletonize_blocks"]["trees_kept"] = int(sum((s[1] == -1).sum() for s in forests.values()))
    report["skeletonize_blocks"]["vertices"] = int(sum(len(s[1]) for s in forests.values()))
    print(json.dumps(report["skeletonize_blocks"]), flush=True)
    whole = {}
    report["skeletonize_pieces"] = {
        "ms": median_ms(lambda: whole.update(inference.skeletonize_pieces(labels))),
        "trees": int(sum((s[1] == -1).sum() for s in whole.values())),
        "vertices": int(sum(len(s[1]) for s in whole.values())),
    }
    report["blocks_over_whole"] = round(report["skeletonize_blocks"]["ms"] / report["skeletonize_pieces"]["ms"], 3)
    text = json.dumps(report, indent=1)
    print(text)
    out = args.out or os.path.join(ROOT, "profiles", f"skeletonize_blocks_{n}.json")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
