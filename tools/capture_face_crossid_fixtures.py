"""Authoring machine only: write tests/golden/g12_face_crossid.npz, the reference's key-point preparation of the two cross-identity demo pairs
(test114 -> val024 and val024 -> test114: subject -> driver) and the label maps it leads to.

The reference's dataset/dataset_video_face.py is imported unmodified, behind empty stand-ins for the modules that FaceDatasetTest's key-point
methods never touch and this environment may lack (cv2, skimage, torchvision.transforms.functional, imageio, json_tricks).  Starting from the
crop-relative landmarks of the two clips stored in tests/golden/g7_raster_face.npz (what read_keypoints returns with fix_crop_pos=True), the
steps of FaceDatasetTest.__getitem__ between reading the landmarks and resizing the maps run as the loader runs them:

    normalize_faces(subject, is_ref=True)  (:335)      -> ref_dist_x / ref_dist_y of the 38 groups, img_scale: the 77 statistics
    normalize_faces(driver, is_ref=False)  (:355)      -> the adapted points
    the five-frame moving average          (:357-379)  -> the smoothed points (the lines are restated here: they are inline in __getitem__)
    get_face_image / get_bbox_image        (:394-395)  -> edge map and bounding-box mask of every driving frame at crop resolution

Stored, data only: per pair the statistics, the adapted and the smoothed points (float64), the maps bit-packed as in g7, and metadata.

    python tools/capture_face_crossid_fixtures.py /path/to/reference
"""
import json
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
PAIRS = [("test114", "val024"), ("val024", "test114")]           # (subject, driver): the pairs of the g10 face goldens
IMG_MEAN = np.array((101.84807705937696, 112.10832843463207, 111.65973036298041), dtype=np.float32)


def import_reference_dataset(ref):
    for name in ("cv2", "skimage", "skimage.transform", "torchvision", "torchvision.transforms", "torchvision.transforms.functional",
                 "imageio", "json_tricks"):
        m = types.ModuleType(name)
        if name in ("torchvision", "torchvision.transforms", "skimage"):
            m.__path__ = []                                        # packages
        sys.modules[name] = m
    sys.modules["skimage"].img_as_bool = None                      # imported by name, never called by the methods used here
    sys.modules["skimage.transform"].resize = None
    sys.modules["skimage.transform"].rescale = None
    sys.path.insert(0, ref)
    import dataset.dataset_video_face as ds
    return ds


def moving_average(frames):
    """dataset_video_face.py:357-379, the statements of __getitem__ on a list of (68,2) arrays -> list of (68,2) arrays"""
    stacked = np.stack(frames, axis=0)
    out = []
    for iky in range(stacked.shape[1]):
        cur = stacked[:, iky, :]
        cumsum = np.cumsum(cur, axis=0)
        win_len = 5
        num_frame = cur.shape[0]
        new = np.zeros_like(cur)
        new[0] = cumsum[0]
        new[1] = cumsum[2] / 3
        new[2] = cumsum[4] / 5
        for ii in range(3, num_frame - 2):
            new[ii] = (cumsum[ii + 2] - cumsum[ii - 3]) / win_len
        new[num_frame - 2] = (cumsum[-1] - cumsum[-4]) / 3
        new[num_frame - 1] = cur[-1]
        out.append(new)
    return [np.array(x) for x in np.stack(out, axis=1).tolist()]


def main():
    ds = import_reference_dataset(sys.argv[1])
    z7 = np.load(os.path.join(GOLD, "g7_raster_face.npz"))
    clips = json.loads(str(z7["meta"]))["clips"]
    arrays, meta = {}, {"pairs": {}, "source": "tests/golden/g7_raster_face.npz key points through dataset/dataset_video_face.py", "numpy": np.__version__}
    for subject, driver in PAIRS:
        d = ds.FaceDatasetTest(None, None, None, None, mean=IMG_MEAN, fix_crop_pos=True)
        sub = [k.copy() for k in z7[f"{subject}_keypoints"]]
        drv = [k.copy() for k in z7[f"{driver}_keypoints"]]
        d.normalize_faces(sub, is_ref=True)                                                     # :335
        stats = np.array([float(v) for v in d.ref_dist_x[:38]] + [float(v) for v in d.ref_dist_y[:38]] + [float(d.img_scale)], dtype=np.float64)
        assert all(np.array_equal(a, b) for a, b in zip(sub, z7[f"{subject}_keypoints"]))       # the subject clip is only measured
        adapted = np.stack(d.normalize_faces(drv, is_ref=False))                                 # :355
        smoothed = moving_average(list(adapted))
        c = clips[driver]
        size, bw = tuple(c["size"]), c["bw"]                                                    # PIL (w, h) of the driving crop; tar_bw (:347)
        edges = np.stack([d.get_face_image(k, size, bw=bw) for k in smoothed])                  # :394
        boxes = np.stack([d.get_bbox_image(k, size) for k in smoothed])                         # :395
        smoothed = np.stack(smoothed)
        assert set(np.unique(edges)) <= {0, 255} and set(np.unique(boxes)) <= {0, 255}
        raw = z7[f"{driver}_keypoints"]
        raw_edges = np.unpackbits(z7[f"{driver}_edges"], axis=-1)[:, :, :size[0]] * 255
        name = f"{subject}_to_{driver}"
        arrays[f"{name}_stats"] = stats
        arrays[f"{name}_adapted"] = adapted.astype(np.float64)
        arrays[f"{name}_smoothed"] = smoothed.astype(np.float64)
        arrays[f"{name}_edges"] = np.packbits(edges > 0, axis=-1)
        arrays[f"{name}_bbox"] = np.packbits(boxes > 0, axis=-1)
        meta["pairs"][name] = dict(subject=subject, driver=driver, frames=int(adapted.shape[0]), crop=c["crop"], subject_crop=clips[subject]["crop"],
                                   bw=int(bw), size=[int(size[0]), int(size[1])],
                                   max_shift_px=float(np.abs(adapted - raw).max()),
                                   fractional_share=float((smoothed != np.floor(smoothed)).mean()),
                                   frames_equal_to_raw_map=int(sum(np.array_equal(a, b) for a, b in zip(edges, raw_edges))),
                                   edge_pixels=int((edges > 0).sum()), bbox_pixels=int((boxes > 0).sum()))
        print(f"[{name}] {meta['pairs'][name]}")
    out = os.path.join(GOLD, "g12_face_crossid.npz")
    np.savez_compressed(out, meta=json.dumps(meta), **arrays)
    print("saved", os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
