"""Kernel by kernel, what `make -C sharkmer_amd/csrc asm` says of two builds of shk_engine.hip — a parent commit's and
this one's: the compiler's resource report (its stderr, -Rpass-analysis=kernel-resource-usage) and a SHA-256 of every
kernel's instruction stream from shk_engine.s, with block labels renumbered and comments dropped (a function's position
in the file numbers its labels, so a new kernel renumbers those of every kernel after it).

    make -C sharkmer_amd/csrc asm 2> this.log      # on each commit; keep shk_engine.s beside the log
    python3 tools/asm_compare.py parent.log parent.s this.log this.s --out profiles/NAME_asm.json

A kernel "differs" when its resources or its instruction hash do."""
import argparse
import hashlib
import json
import re

FIELDS = ("TotalSGPRs", "VGPRs", "AGPRs", "ScratchSize", "Occupancy", "SGPRs Spill", "VGPRs Spill", "LDS Size")


def resources(log_path):
    out, cur = {}, None
    for line in open(log_path, errors="replace"):
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            cur = out.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\d+)", line)
        if m and cur is not None and m.group(1) in FIELDS:
            cur[m.group(1)] = int(m.group(2))
    return out


def instruction_hashes(asm_path):
    out, cur = {}, None
    for line in open(asm_path, errors="replace"):
        m = re.match(r"^(_Z\w+):", line)
        if m:
            cur = out.setdefault(m.group(1), hashlib.sha256())
            continue
        if cur is None:
            continue
        if line.startswith(".Lfunc_end"):
            cur = None
            continue
        line = line.split(";")[0].rstrip()
        line = re.sub(r"LBB\d+_", "LBB_", line)
        line = re.sub(r"\.Ltmp\d+", ".Ltmp", line)
        if not line or line.lstrip().startswith((".loc", ".file", ".cfi", ".Ltmp")):
            continue
        cur.update(line.encode() + b"\n")
    return {k: h.hexdigest() for k, h in out.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("parent_log")
    ap.add_argument("parent_asm")
    ap.add_argument("this_log")
    ap.add_argument("this_asm")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    pr, tr = resources(a.parent_log), resources(a.this_log)
    ph, th = instruction_hashes(a.parent_asm), instruction_hashes(a.this_asm)
    kernels = {}
    for name in sorted(set(pr) | set(tr)):
        kernels[name] = {"parent": dict(pr[name], instructions_sha256=ph.get(name)) if name in pr else None,
                         "this": dict(tr[name], instructions_sha256=th.get(name)) if name in tr else None}
    both = [n for n, v in kernels.items() if v["parent"] and v["this"]]
    res = {"what": "make asm (gfx950) of every kernel of shk_engine.hip, parent commit and this one: the compiler's resource report "
                   "and a SHA-256 of the kernel's instructions with block labels renumbered and comments dropped (tools/asm_compare.py)",
           "n_kernels_parent": len(pr), "n_kernels_this": len(tr),
           "kernels_that_differ": [n for n in both if kernels[n]["parent"] != kernels[n]["this"]],
           "kernels_new": [n for n, v in kernels.items() if v["parent"] is None],
           "kernels_gone": [n for n, v in kernels.items() if v["this"] is None],
           "kernels": kernels}
    text = json.dumps(res, indent=1) + "\n"
    if a.out:
        open(a.out, "w").write(text)
    print(json.dumps({k: res[k] for k in ("n_kernels_parent", "n_kernels_this", "kernels_that_differ", "kernels_new", "kernels_gone")}))


if __name__ == "__main__":
    main()
