#!/usr/bin/env python3
"""Worst error per stratum of the device's Box-Muller transform (box_muller_raw, pair_sum_raw) and of sqrt_nonneg against the fp64
reference, through the instrumented build's taps (olmc_box_muller_probe, olmc_sqrt_nonneg_probe) -- the inputs, strata and measuring
code of tests/box_muller_reference.py, i.e. exactly what tests/test_gpu_box_muller.py gates.

    python tools/box_muller_accuracy.py [--out FILE.jsonl]

One JSON line per (input set, stratum, output): `ratio` = kZScale |device - reference| / max(1, kZScale rad) at the worst draw (the
gate is ratio <= 2e-5), `abs_err` in RAW units and the words (xa, xb) of that draw; one line per range of the square root: worst
error in ulp, relative and absolute against numpy.sqrt."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import box_muller_reference as bm  # noqa: E402
from tools.probe import binding as probe  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = []
    sets = (("angle_sweep_rad_1", bm.measure_angle_sweep(probe.box_muller_probe)),
            ("radius_edges_x_angles", bm.measure_radius_cross(probe.box_muller_probe, bm.radius_edge_words())),
            ("radius_strided_x_angles", bm.measure_radius_cross(probe.box_muller_probe, bm.radius_strided_words())))
    for name, m in sets:
        flags = {k: m[k] for k in ("finite", "upper_bits_ignored", "zeros_at_one")}
        for stratum, outputs in m["worst"].items():
            for output, w in outputs.items():
                lines.append(dict(what="box_muller", inputs=name, stratum=stratum, output=output, gate=bm.Z_ABS_TOL, **w, **flags))
    for name, m in bm.measure_sqrt(probe.sqrt_nonneg_probe).items():
        lines.append(dict(what="sqrt_nonneg", range=name, **m))
    lines.append(dict(what="device", **probe.hip.device_info()))
    text = "".join(json.dumps(line) + "\n" for line in lines)
    sys.stdout.write(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
