"""Rotated ground truth from a polygon COCO json: the reference's tools/mask_to_rbox.py without OpenCV.

    python tools/mask_to_rbox.py input.json output.json [--device cuda|cpu] [--skip-crowd | --keep-crowd]

Every non-crowd annotation's ``bbox`` becomes the five numbers (cx, cy, w, h, angle_deg) of the canonical minimum-area rectangle of
its polygons (slenderobjdet_amd/data/rotated_coco.py); all rectangles come from one kernel launch on ``--device cuda``, from the numpy
path on ``cpu``.  Crowd annotations are dropped when the input's name contains "val", as the reference does, unless a flag says
otherwise.  RotatedCOCOEvaluator reads the output as it is.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from slenderobjdet_amd.data.rotated_coco import coco_to_rotated  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("input")
    ap.add_argument("output")
    ap.add_argument("--device", default="cuda", choices=["cuda", "cpu"])
    crowd = ap.add_mutually_exclusive_group()
    crowd.add_argument("--skip-crowd", dest="skip_crowd", action="store_true", default=None, help="drop crowd annotations")
    crowd.add_argument("--keep-crowd", dest="skip_crowd", action="store_false", help="keep crowd annotations as [x, y, w, h, 0]")
    a = ap.parse_args(argv)
    skip = ("val" in os.path.basename(a.input)) if a.skip_crowd is None else a.skip_crowd
    with open(a.input) as f:
        dataset = json.load(f)
    out = coco_to_rotated(dataset, skip_crowd=skip, device=a.device)
    out["info"]["description"] = f"Rotated-box (cx, cy, w, h, angle_deg) version of {os.path.basename(a.input)}: minimum-area rectangles of the polygons."
    with open(a.output, "w") as f:
        json.dump(out, f)
    print(f"{len(out['annotations'])} of {len(dataset.get('annotations', []))} annotations written to {a.output}")


if __name__ == "__main__":
    main()
