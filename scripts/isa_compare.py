"""Device assembly of csrc/*.hip at a parent commit against the working tree, for refactors that must not change the kernels.

  python scripts/isa_compare.py [--parent HEAD] [--out profiles/NAME.md] nerf_fwd nerf_fwd_bf16 ...

Each named source is compiled twice with the product flags (nerfmatch_amd.build.FLAGS) plus `-S --cuda-device-only` -- once from
`git archive PARENT` unpacked into a temporary directory, once from the tree.  The assembly is normalised (comment lines, .file / .loc /
.ident and the per-compilation __hip_cuid_* symbol dropped) and compared kernel by kernel (label to end of function, the kernel
descriptor included); per kernel the resource counts of the code object's metadata are listed for both sides.  Needs hipcc, no GPU.  Prints a markdown table (and writes it to --out).
"""
import argparse
import os
import re
import subprocess
import sys
import tempfile
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
from nerfmatch_amd import build  # noqa: E402

FIELDS = ("vgpr_count", "agpr_count", "sgpr_count", "group_segment_fixed_size", "private_segment_fixed_size", "vgpr_spill_count")


def assembly(root, stem):
    src = root / "nerfmatch_amd" / "csrc" / f"{stem}.hip"
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    r = subprocess.run([hipcc, *build.FLAGS, "-S", "--cuda-device-only", str(src), "-o", "-"], capture_output=True, text=True)
    if r.returncode:
        sys.exit(r.stderr)
    return r.stdout


def normalised(asm):
    keep = []
    for line in asm.splitlines():
        t = line.strip()
        if not t or t.startswith(";") or t.startswith("//") or re.match(r"\.(file|loc|ident)\b", t) or "__hip_cuid_" in t:
            continue
        keep.append(re.sub(r"\s*;.*$", "", line.rstrip()))
    return keep


def kernels(asm):
    """one metadata entry per kernel: entries start with a list item at the indentation of amdhsa.kernels' children"""
    meta = asm[asm.find("amdhsa.kernels:"):].split("amdhsa.target:")[0]
    out = {}
    for entry in re.split(r"\n  - ", meta)[1:]:
        name = re.search(r"^\s*\.name:\s*(\S+)", entry, re.M)
        vals = {f: int(m.group(1)) for f in FIELDS if (m := re.search(rf"^\s*\.{f}:\s*(\d+)", entry, re.M))}
        if name:
            out[name.group(1)] = vals
    return out


def body(lines, name):
    """the normalised lines of one kernel: from its label to the end of its function, kernel descriptor included"""
    a = lines.index(name + ":")
    return lines[a:next(i for i in range(a, len(lines)) if lines[i].startswith(".Lfunc_end"))]


def verdict(a, b):
    if a == b:
        return f"identical ({len(a)} lines)"
    return f"same lines in another order ({len(a)} lines)" if sorted(a) == sorted(b) else f"differs ({len(a)} -> {len(b)} lines)"


def short(name):
    r = subprocess.run(["c++filt", name], capture_output=True, text=True)
    d = r.stdout.strip() if r.returncode == 0 and r.stdout.strip() else name
    return re.sub(r"^\(anonymous namespace\)::|\(.*$", "", re.sub(r"^void ", "", d))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("stems", nargs="+")
    ap.add_argument("--parent", default="HEAD")
    ap.add_argument("--out")
    a = ap.parse_args()
    rev = subprocess.run(["git", "-C", str(ROOT), "rev-parse", "--short", a.parent], capture_output=True, text=True, check=True).stdout.strip()
    lines = [f"Device assembly, parent `{rev}` against the tree; flags `{' '.join(build.FLAGS)} -S --cuda-device-only`.", "",
             "| unit | kernel | normalised assembly | " + " | ".join(f.replace("_fixed_size", "").replace("_count", "") for f in FIELDS) + " |",
             "|---|---|---|" + "---|" * len(FIELDS)]
    with tempfile.TemporaryDirectory() as tmp:
        tar = subprocess.run(["git", "-C", str(ROOT), "archive", a.parent, "nerfmatch_amd/csrc", "include"], capture_output=True, check=True).stdout
        subprocess.run(["tar", "-x", "-C", tmp], input=tar, check=True)
        for stem in a.stems:
            pa, br = assembly(Path(tmp), stem), assembly(ROOT, stem)
            na, nb = normalised(pa), normalised(br)
            kp, kb = kernels(pa), kernels(br)
            assert set(kp) == set(kb), (sorted(kp), sorted(kb))
            for k in sorted(kp):
                cells = [str(kp[k].get(f)) if kp[k].get(f) == kb[k].get(f) else f"**{kp[k].get(f)} -> {kb[k].get(f)}**" for f in FIELDS]
                lines.append(f"| `{stem}.hip` | `{short(k)}` | {verdict(body(na, k), body(nb, k))} | " + " | ".join(cells) + " |")
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        Path(a.out).write_text(text)


if __name__ == "__main__":
    main()
