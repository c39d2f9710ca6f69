#!/usr/bin/env python3
"""Which kernels of two builds have the same device code, and the resources of those that do not (no GPU needed).
    python tools/kernel_text_diff.py PARENT/olmc.s NEW/olmc.s [--out FILE.json]
Each argument is the device assembly tools/kernel_meta.sh leaves (its hipcc -S --cuda-device-only line, run in either tree).  A kernel's
text is its function body with comments stripped and the `.LBB<n>_` label prefixes normalised.  For a changed kernel `resources_hold`
says that both builds have no scratch and no VGPR spills, the same LDS bytes, the same SGPR class (allocation granule 16), the same VGPR
allocation row (granule 8) and so the same waves per SIMD (512 registers per lane, at most 8).  `sspill` counts SGPRs spilled to VGPR
lanes (no memory traffic); it is reported, not part of the flag."""
import argparse
import json
import re
import subprocess


def kernels(path):
    """{demangled name: (text lines, resources)} of one assembly file."""
    txt = open(path).read()
    meta = {}
    for b in re.split(r"\n  - \.", txt[txt.rfind("amdhsa.kernels"):])[1:]:
        g = lambda k: (re.search(r"\.%s:\s+(\S+)" % k, b) or [None, None])[1]
        if g("name"):
            meta[g("name")] = dict(vgpr=int(g("vgpr_count")), sgpr=int(g("sgpr_count")), lds=int(g("group_segment_fixed_size")),
                                   scratch=int(g("private_segment_fixed_size")), spill=int(g("vgpr_spill_count")), sspill=int(g("sgpr_spill_count")))
    names = subprocess.run(["c++filt"], input="\n".join(meta), capture_output=True, text=True).stdout.split("\n")
    out = {}
    for sym, dem in zip(meta, names):
        body = txt[txt.index("\n%s:" % sym):]
        body = body[:body.index(".Lfunc_end")]
        lines = [re.sub(r"\.LBB\d+_", ".LBB_", re.sub(r"\s*;.*", "", l)).strip() for l in body.split("\n")[2:]]
        out[re.sub(r"\(.*", "", dem).replace("void olmc::", "")] = ([l for l in lines if l], meta[sym])
    return out


def waves(r):
    return min(8, 512 // (-(-r["vgpr"] // 8) * 8))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("parent")
    ap.add_argument("new")
    ap.add_argument("--out")
    a = ap.parse_args()
    old, new = kernels(a.parent), kernels(a.new)
    changed = []
    for name in sorted(set(old) & set(new)):
        (t0, r0), (t1, r1) = old[name], new[name]
        if t0 == t1:
            continue
        hold = (all(r["scratch"] == 0 and r["spill"] == 0 for r in (r0, r1)) and r0["lds"] == r1["lds"] and -(-r0["sgpr"] // 16) == -(-r1["sgpr"] // 16)
                and -(-r0["vgpr"] // 8) == -(-r1["vgpr"] // 8) and waves(r0) == waves(r1))
        changed.append(dict(kernel=name, lines=[len(t0), len(t1)], parent=r0, new=r1, waves_per_simd=[waves(r0), waves(r1)], resources_hold=hold))
    doc = dict(kernels=len(new), only_parent=sorted(set(old) - set(new)), only_new=sorted(set(new) - set(old)),
               same=len(set(old) & set(new)) - len(changed), changed=changed)
    for c in changed:
        f = lambda r: "%3d v %3d s %5d lds %d scratch %d spill %3d sspill" % (r["vgpr"], r["sgpr"], r["lds"], r["scratch"], r["spill"], r["sspill"])
        print("%-44s %s -> %s  %s" % (c["kernel"], f(c["parent"]), f(c["new"]), "holds" if c["resources_hold"] else "LEAVES"))
    print("%d kernels, %d same, %d changed" % (doc["kernels"], doc["same"], len(changed)))
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(doc, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
