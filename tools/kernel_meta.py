"""Register / spill / LDS figures of the kernels in a built library (no GPU needed):
    python tools/kernel_meta.py [--hash] [path/to/lib.so] [regex]
Reads the code-object metadata the way tests/test_kernel_budget.py does. --hash adds a SHA-256 of
each kernel's disassembly without addresses and encodings: two builds whose lines agree compiled
the same kernels (profiles/conv_prune_kernel_identity.txt)."""
import hashlib
import os
import re
import subprocess
import sys
import tempfile

import yaml

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = "/opt/rocm/lib/llvm/bin"


def disassembly(co):
    """{mangled name: instruction lines} of a code object: the text left of llvm-objdump's
    "// address: encoding" comments."""
    text = subprocess.run([f"{LLVM}/llvm-objdump", "-d", "--mcpu=gfx950", co], check=True,
                          capture_output=True, text=True).stdout
    out, cur = {}, None
    for line in text.split("\n"):
        m = re.match(r"[0-9a-f]+ <(.+)>:$", line)
        if m:
            cur = out.setdefault(m.group(1), [])
        elif cur is not None and line.startswith("\t"):
            cur.append(line.split("//")[0].strip())
    return out


def kernels(lib, asm=False):
    found = {}
    with tempfile.TemporaryDirectory() as tmp:
        fat = os.path.join(tmp, "fat.bin")
        subprocess.run([f"{LLVM}/llvm-objcopy", f"--dump-section=.hip_fatbin={fat}", lib,
                        os.path.join(tmp, "ignored.so")], check=True)
        data = open(fat, "rb").read()
        starts = [m.start() for m in re.finditer(b"__CLANG_OFFLOAD_BUNDLE__", data)]
        for i, p in enumerate(starts):
            piece = os.path.join(tmp, f"b{i}.bin")
            with open(piece, "wb") as f:
                f.write(data[p:starts[i + 1] if i + 1 < len(starts) else len(data)])
            co = os.path.join(tmp, f"b{i}.co")
            subprocess.run([f"{LLVM}/clang-offload-bundler", "--unbundle", "--type=o",
                            "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--input={piece}",
                            f"--output={co}"], check=True)
            notes = subprocess.run([f"{LLVM}/llvm-readelf", "--notes", co], check=True,
                                   capture_output=True, text=True).stdout
            body = notes.split("---", 1)[1].rsplit("...", 1)[0]
            dis = disassembly(co) if asm else {}
            for k in yaml.safe_load(body)["amdhsa.kernels"]:
                found[k[".name"]] = k
                if asm:
                    k["asm"] = dis[k[".name"]]
    names = list(found)
    plain = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True,
                           check=True).stdout.split("\n")
    return {p: found[n] for n, p in zip(names, plain)}


if __name__ == "__main__":
    args = [x for x in sys.argv[1:] if x != "--hash"]
    want_hash = "--hash" in sys.argv
    lib = args[0] if args else os.path.join(
        ROOT, "aind_exaspim_neuron_segmentation_amd", "csrc", "libexaspim_affinity.so")
    pat = args[1] if len(args) > 1 else "."
    for name, k in sorted(kernels(lib, asm=want_hash).items()):
        if re.search(pat, name):
            short = name.replace("exaspim::", "").replace("(ConvArgs, int, int, int)", "").replace("void ", "")
            if want_hash:   # the whole name: the line identifies the kernel
                print(f"{name}  sha256 {hashlib.sha256(chr(10).join(k['asm']).encode()).hexdigest()}  ", end="")
            else:
                print(f"{short[:90]:90s} ", end="")
            print(f"vgpr {k['.vgpr_count']:4d} spills {k['.vgpr_spill_count']:3d} "
                  f"sgpr-spills {k['.sgpr_spill_count']:3d} scratch {k['.private_segment_fixed_size']:4d} "
                  f"lds {k['.group_segment_fixed_size']}")
