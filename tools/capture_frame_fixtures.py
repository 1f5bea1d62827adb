"""Authoring machine only: write tests/golden/g11_frames_<clip>.npz, the INPUT side of the frame loader's parity test.

For the four source clips of the g10 goldens this stores the cropped uint8 RGB region (Image.crop semantics: zeros outside the frame) of the
three source frames and the crop box.  The crop boxes come from the raster goldens' metadata (g7 / g9), the pixels from the reference's demo
image files; nothing of the reference's code is imported.  The expected outputs are the `in_src_bgr` bytes already stored with the g10 goldens
(oracle/capture_demo_input_goldens.py).

    python tools/capture_frame_fixtures.py /path/to/reference
"""
import json
import os
import sys

import numpy as np
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
# (clip, model, frame indices) -- the sources of the four g10 pairs
CLIPS = [("test114", "face", (0, 13, 26)), ("val024", "face", (0, 12, 24)), ("00110", "pose", (0, 10, 20)), ("00164", "pose", (0, 10, 20))]


def main():
    ref = sys.argv[1]
    z7 = json.loads(str(np.load(os.path.join(GOLD, "g7_raster_face.npz"))["meta"]))
    z9 = json.loads(str(np.load(os.path.join(GOLD, "g9_raster_pose.npz"))["meta"]))
    for clip, model, idx in CLIPS:
        if model == "face":
            c = z7["clips"][clip]
            ys, ye, xs, xe = c["crop"]                                        # get_crop_coords order
            box = (xs, ys, xe, ye)
            paths = [os.path.join(ref, "demo", "face_examples", "images", clip, c["files"][f].replace(".txt", ".png")) for f in idx]
        else:
            c = z9["clips"][clip]
            box = tuple(c["crop"])
            paths = [os.path.join(ref, "demo", "dance_example", "images", clip, c["files"][f].replace("_keypoints.json", ".jpg")) for f in idx]
        ims = [Image.open(p).convert("RGB") for p in paths]
        crops = np.stack([np.asarray(im.crop(box)) for im in ims])
        meta = dict(clip=clip, model=model, frames=list(idx), box=[int(v) for v in box], frame_size=list(ims[0].size),
                    files=[os.path.basename(p) for p in paths])
        out = os.path.join(GOLD, f"g11_frames_{clip}.npz")
        np.savez_compressed(out, meta=json.dumps(meta), crops=crops)
        print(f"[{clip}] box {box} of {ims[0].size}, crops {crops.shape}, {os.path.getsize(out)} bytes")


if __name__ == "__main__":
    main()
