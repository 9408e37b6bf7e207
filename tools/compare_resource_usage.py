#!/usr/bin/env python3
"""Compare two listings of ``make -C keypoints2body_amd/csrc resource-usage`` (clang's -Rpass-analysis=kernel-resource-usage).

    python tools/compare_resource_usage.py profiles/resource_usage_parent.txt profiles/resource_usage_branch.txt

Every kernel that both listings name must show the same figures; kernels of one listing alone are printed with theirs.  Exit
status 1 if a shared kernel differs."""
import re
import sys

FIELDS = ("TotalSGPRs", "VGPRs", "AGPRs", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]", "SGPRs Spill", "VGPRs Spill",
          "LDS Size [bytes/block]")


def parse(path):
    kernels, name = {}, None
    for line in open(path):
        m = re.search(r"remark:\s+(.*?): (\S+) \[-Rpass-analysis", line)
        if not m:
            continue
        key, value = m.group(1).strip(), m.group(2)
        if key == "Function Name":
            name = value
            kernels[name] = {}
        elif name is not None and key in FIELDS:
            kernels[name][key] = value
    return kernels


def main(parent_path, branch_path):
    parent, branch = parse(parent_path), parse(branch_path)
    shared = [k for k in parent if k in branch]
    differ = [k for k in shared if parent[k] != branch[k]]
    print(f"{len(parent)} kernels in {parent_path}, {len(branch)} in {branch_path}, {len(shared)} in both, {len(differ)} differ")
    for k in differ:
        print("DIFFERS", k, parent[k], branch[k])
    for k in parent:
        if k not in branch:
            print("GONE   ", k)
    for k in branch:
        if k not in parent:
            f = branch[k]
            print("NEW    ", k, "VGPRs", f["VGPRs"], "SGPRs", f["TotalSGPRs"], "scratch", f["ScratchSize [bytes/lane]"], "LDS", f["LDS Size [bytes/block]"],
                  "occupancy", f["Occupancy [waves/SIMD]"], "VGPR spills", f["VGPRs Spill"], "SGPR spills", f["SGPRs Spill"])
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main(*sys.argv[1:3]))
