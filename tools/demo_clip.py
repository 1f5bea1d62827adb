"""Demo clip harness (the caller pattern of demo/demo_face.py:108-236) on one MI355X:

    checkpoint dict -> TSNet(n_blocks=4) -> key points of a synthetic talking-head clip -> label maps ON THE DEVICE (rank 3 kernels)
    -> set_sources once -> per driving frame: forward_target (batch 1) + device post-processing -> strips (PNG) + clip (GIF)

and the demo-shaped throughput figure (B=1, n_blocks=4, K=3, clip mode).  No pretrained checkpoint is reachable from this image
(README.md:36-39 links to Google Drive), so the checkpoint is a randomly initialised generator saved and re-loaded through the
reference's .pth schema {'img_enc','lbl_enc','dec','fuse_net'} (train_face.py:350-355): the frames are noise, the path is the real one.

    python tools/demo_clip.py --out gpurun_out/demo --frames 16

Cross-identity (demo/demo_face.py with different subject and driving clips): `--clip SUBJECT --drive DRIVER` takes the source pixels and labels
from SUBJECT and the driving labels from DRIVER's key points as the reference's loader prepares them -- adapted to the subject's face proportions
and smoothed over the clip (raster.face_driving_keypoints), then drawn from the fractional points (rasterise(relative=True)).

    python tools/demo_clip.py --out demo_out --clip test114 --drive val024 --frames 16

`--compact` hands the runner the compact form of every input -- image bytes before the mean subtraction, class maps, byte masks (a quarter of the
bytes and less) -- and must write the same files, byte for byte.

`--paste-back` also puts every generated frame back into the full video frame at the clip's crop box on the device (FrameLoader.paste_face) and
writes "<i>_<name>_full.png".  The goldens hold key points and the cropped source regions only, no driving frames, so the frames pasted into are
synthetic (a gradient of the clip's frame size); the tool says so.

`--track-crop` crops every frame by the box of its own landmarks, as the reference's FaceDatasetTest(fix_crop_pos=False) does: source and driving
labels are drawn at each frame's own crop (raster.crop_coords_clip, FaceRasteriser.clip_labels(crop=(F,4))), with `--drive` the driving key points
are made relative to their own crops before adaptation and smoothing (face_driving_keypoints(fix_crop_pos=False)), and with `--paste-back` every
generated frame goes back at its own box (ClipRunner.run(paste_boxes=...), one launch per group).  It composes with --drive, --compact and --batch.
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from wacv23_tsnet_amd import demo, raster
from wacv23_tsnet_amd.model import TSNet


def synthetic_face_keypoints(n_frames: int, seed: int = 0) -> np.ndarray:
    """68 landmarks of a schematic face in a 640 x 480 frame (the demo clips' size) that nods and opens its mouth: (F,68,2) integers."""
    t = np.linspace(0, 2 * np.pi, n_frames, endpoint=False)
    out = np.zeros((n_frames, 68, 2))
    for f, ph in enumerate(t):
        cx, cy, s = 320 + 12 * np.sin(ph), 240 + 8 * np.cos(ph), 70.0
        a = np.linspace(np.pi * 0.05, np.pi * 0.95, 17)
        out[f, 0:17] = np.stack([cx - 1.05 * s * np.cos(a), cy - 0.1 * s + 1.25 * s * np.sin(a)], 1)          # contour
        for k, (x0, x1) in enumerate(((-0.8, -0.2), (0.2, 0.8))):                                            # eyebrows
            xs = np.linspace(x0, x1, 5)
            out[f, 17 + 5 * k:22 + 5 * k] = np.stack([cx + s * xs, cy - 0.55 * s - 0.12 * s * np.sin(np.pi * (xs - x0) / (x1 - x0))], 1)
        out[f, 27:31] = np.stack([np.full(4, cx), cy - 0.35 * s + np.linspace(0, 0.45 * s, 4)], 1)           # nose bridge
        out[f, 31:36] = np.stack([cx + s * np.linspace(-0.22, 0.22, 5), cy + 0.2 * s + 0.05 * s * np.sin(np.linspace(0, np.pi, 5))], 1)
        for k, ex in enumerate((-0.5, 0.5)):                                                                 # eyes
            ang = np.linspace(np.pi, -np.pi, 6, endpoint=False)
            out[f, 36 + 6 * k:42 + 6 * k] = np.stack([cx + s * (ex + 0.2 * np.cos(ang)), cy - 0.3 * s - 0.09 * s * np.sin(ang)], 1)
        op = 0.08 + 0.1 * (1 + np.sin(2 * ph)) / 2                                                           # mouth opening
        ang = np.linspace(np.pi, -np.pi, 12, endpoint=False)
        out[f, 48:60] = np.stack([cx + 0.42 * s * np.cos(ang), cy + 0.6 * s - (op + 0.1) * s * np.sin(ang)], 1)
        ang = np.linspace(np.pi, -np.pi, 8, endpoint=False)
        out[f, 60:68] = np.stack([cx + 0.28 * s * np.cos(ang), cy + 0.6 * s - op * s * np.sin(ang)], 1)
    return np.round(out)


def synthetic_frames(n: int, h: int, w: int) -> np.ndarray:
    """(n,h,w,3) uint8: a colour gradient standing in for the video frames that are not at hand"""
    y, x = np.mgrid[0:h, 0:w]
    a = np.stack([x * 255 // max(w - 1, 1), y * 255 // max(h - 1, 1), (x + y) * 255 // max(w + h - 2, 1)], 2).astype(np.uint8)
    return np.ascontiguousarray(np.broadcast_to(a, (n, h, w, 3)))


GOLD = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden")


def clip_keypoints(clip: str):
    """(F,68,2) key points of a real demo clip in FRAME coordinates and the clip's metadata (tests/golden/g7_raster_face.npz stores them
    relative to the clip's crop; the landmark files hold integers, so adding the crop back is exact)"""
    import json
    z = np.load(os.path.join(GOLD, "g7_raster_face.npz"))
    meta = json.loads(str(z["meta"]))["clips"][clip]
    kp = z[f"{clip}_keypoints"].copy()
    kp[:, :, 0] += meta["crop"][2]
    kp[:, :, 1] += meta["crop"][0]
    return kp, meta


def crossid_labels(rs, subject_kps, driving_kps, size=(256, 256), compact=False, track_crop=False):
    """Driving labels of a cross-identity pair, the reference loader's way (dataset/dataset_video_face.py:335-398): the driving clip's key points
    adapted to the subject's face and smoothed (host code of the library), drawn at the driving crop's resolution from the fractional points,
    resized, one-hot.  rs: a raster.FaceRasteriser (its device and library are used throughout).  Key points in frame coordinates.
    Returns (labels (F,2,H,W), bbox (F,H,W), driving crop, bw); compact: the class map (F,H,W) and the mask as uint8.
    track_crop: every frame by its own crop (fix_crop_pos=False); the driving crop returned is then (F,4)."""
    if track_crop:
        pts, crops, bw = raster.face_driving_keypoints(subject_kps, driving_kps, lib=rs.lib, fix_crop_pos=False)
        lbl, box, _ = rs.clip_labels(list(pts), size, crop=crops, relative=True, compact=compact, bw=bw)
        return lbl, box, crops, bw
    pts, crop, bw = raster.face_driving_keypoints(subject_kps, driving_kps, lib=rs.lib)
    edges, bbox, _, _ = rs.rasterise(list(pts), crop, relative=True)
    cls, box = demo.resize_label(edges, size, lib=rs.lib), demo.resize_label(bbox, size, lib=rs.lib)
    if compact:
        return cls.to(torch.uint8), box.to(torch.uint8), crop, bw
    return rs.vl2ch(cls, 2), box, crop, bw


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="gpurun_out/demo")
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--n-blocks", type=int, default=4)
    ap.add_argument("--timing-frames", type=int, default=200)
    ap.add_argument("--batch", type=int, default=1, help="driving frames per forward_target; > 1: the one source set is cached for the whole "
                    "batch (tsnet_set_sources_shared) and the clip runs in groups of this many frames")
    ap.add_argument("--clip", default=None, help="key points of a real demo clip (demo/face_examples/labels/<clip>, stored with the raster golden "
                    "tests/golden/g7_raster_face.npz: test114 or val024) instead of the synthetic face; the source frames' pixels are the clip's own "
                    "(tests/golden/g11_frames_<clip>.npz through the device frame loader)")
    ap.add_argument("--drive", default=None, help="with --clip: a second demo clip whose key points drive the subject given by --clip (cross-identity); "
                    "the driving labels are adapted to the subject's face proportions and smoothed as the reference's loader does")
    ap.add_argument("--compact", action="store_true", help="compact inputs: image bytes, class maps and byte masks, widened by the engine on load "
                    "(tsnet_*_u8); the files written equal those of a run without the flag")
    ap.add_argument("--paste-back", action="store_true", help="paste every generated frame into a full video frame at the clip's crop box on the "
                    "device and write <i>_<name>_full.png; the frames pasted into are synthetic (no driving frames are stored with the goldens)")
    ap.add_argument("--track-crop", action="store_true", help="a crop per frame from that frame's own landmarks (the reference's fix_crop_pos=False) "
                    "for source and driving labels; with --paste-back, a paste box per frame")
    ap.add_argument("--feather", type=float, default=None, metavar="R", help="with --paste-back: a soft seam, the paste mask through Pillow's "
                    "GaussianBlur(R) on the device (FrameLoader.feather_mask)")
    ap.add_argument("--feather-from", choices=("box", "bbox"), default=None, help="with --feather: box (default) = the feathered crop box, one mask "
                    "for the clip; bbox = every driving frame's own bounding-box mask, feathered")
    ap.add_argument("--y4m", default=None, metavar="OUT.y4m", help="also write the clip as a Y4M video file (uncompressed YUV 4:2:0, BT.601 full "
                    "range; ffmpeg -i OUT.y4m out.mp4 takes it): the full frames with --paste-back, the generated frames without; converted on the "
                    "device (FrameLoader.to_yuv420) and downloaded at half the bytes of RGB")
    args = ap.parse_args()
    if (args.feather is not None or args.feather_from is not None) and not args.paste_back:
        ap.error("--feather and --feather-from need --paste-back")
    if args.feather_from is not None and args.feather is None:
        ap.error("--feather-from needs --feather R")
    if args.drive and not args.clip:
        ap.error("--drive needs --clip (the subject)")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    os.makedirs(args.out, exist_ok=True)

    # ---- checkpoint through the reference's .pth schema (demo_face.py:123-129)
    torch.manual_seed(0)
    m0 = TSNet(is_train=False, label_nc=2, n_blocks=args.n_blocks, n_downsampling=3, n_source=3)
    ckpt = {net: getattr(m0, net).state_dict() for net in ("img_enc", "lbl_enc", "dec", "fuse_net")}
    ckpt["example"] = 0
    path = os.path.join(args.out, "TSNet_B0004_S000000.pth")
    torch.save(ckpt, path)
    model = TSNet(is_train=False, label_nc=2, n_blocks=args.n_blocks, n_downsampling=3, n_source=3)
    model.load_checkpoint(torch.load(path, map_location="cpu"))
    model = model.cuda()

    # ---- labels on the device: key points -> edge map / bbox at crop resolution -> 256 x 256 -> one-hot (rank 3 kernels)
    K, F = 3, args.frames
    crop_in = None
    if args.clip:
        import json
        kp, meta = clip_keypoints(args.clip)
        kp_all = kp
        F = min(F, kp.shape[0] - K)
        kp = kp[:F + K]
    else:
        kp = synthetic_face_keypoints(F + K, seed=0)
    rs = raster.FaceRasteriser(dev)
    t0 = time.perf_counter()
    edges, bbox, crop, bw = rs.rasterise(list(kp), crop_in)
    if args.clip:
        assert list(crop) == meta["crop"] and bw == meta["bw"]      # the crop arithmetic reproduces the reference's on the real clip
    onehot = (lambda m: m.to(torch.uint8)) if args.compact else (lambda m: rs.vl2ch(m, 2))      # compact: the class map itself, no one-hot planes
    mask = (lambda m: m.to(torch.uint8)) if args.compact else (lambda m: m)
    lbl = onehot(demo.resize_label(edges))                       # vl2ch(label map, "face") (demo_face.py:158,164)
    box = mask(demo.resize_label(bbox))
    torch.cuda.synchronize()
    t_raster = time.perf_counter() - t0
    # the first call pays one-off costs (the library's first kernel launches, the caching allocator's first blocks, torch's first
    # index kernels): time the steady state separately, stage by stage
    t_steps = {}
    for _ in range(3):
        ta = time.perf_counter(); e2, b2, _, _ = rs.rasterise(list(kp), crop_in); torch.cuda.synchronize()
        tb = time.perf_counter(); l2 = demo.resize_label(e2); x2 = demo.resize_label(b2); torch.cuda.synchronize()
        tc = time.perf_counter(); rs.vl2ch(l2, 2); torch.cuda.synchronize()
        td = time.perf_counter()
        t_steps = {"fit (host) + draw (device)": tb - ta, "resize 2 maps": tc - tb, "one-hot": td - tc}
    assert torch.equal(e2, edges) and torch.equal(b2, bbox)
    tcrops = None
    if args.track_crop:                                          # the labels again, every frame at its own crop
        tcrops = raster.crop_coords_clip(kp)
        lbl, box, _ = rs.clip_labels(list(kp), crop=tcrops, compact=args.compact)
        print(f"[demo_clip] --track-crop: {len(tcrops)} crops of {sorted({int(c[1] - c[0]) for c in tcrops})} pixels, "
              f"corners moving by up to {int(np.abs(tcrops - tcrops[0]).max())} pixels")
    if args.clip:
        # the real source frames: the cropped regions of the clip's demo images (tests/golden/g11_frames_<clip>.npz) through the device frame
        # loader, and the labels of the SAME frame indices, so that pixels and labels belong together
        from wacv23_tsnet_amd import frames as frames_mod
        zf = np.load(os.path.join(GOLD, f"g11_frames_{args.clip}.npz"))
        fmeta = json.loads(str(zf["meta"]))
        x0, y0, x1, y1 = fmeta["box"]
        assert [y0, y1, x0, x1] == list(crop)
        src_kp = kp_all[[int(i) for i in fmeta["frames"]][:K]]
        if args.track_crop:
            # each source frame by its own crop; the stored pixels are the clip-crop's region only, so what a frame's crop has outside it reads 0
            scrops = raster.crop_coords_clip(src_kp)
            img = frames_mod.FrameLoader(dev).face(zf["crops"][:K], scrops - np.array([y0, y0, x0, x0]), as_bytes=args.compact)
            src_lbl, src_box, _ = rs.clip_labels(list(src_kp), crop=scrops, compact=args.compact)
        else:
            img = frames_mod.FrameLoader(dev).face(zf["crops"], [0, y1 - y0, 0, x1 - x0], as_bytes=args.compact)
            se, sb, _, _ = rs.rasterise(list(src_kp), crop)
            src_lbl, src_box = onehot(demo.resize_label(se)), mask(demo.resize_label(sb))
        src_img = [img[i:i + 1] for i in range(K)]
    else:
        # noise frames of BYTE values, as every decoded frame is: the float form is byte - IMG_MEAN, the compact form the byte
        g = torch.Generator().manual_seed(1)
        src_byte = [(torch.rand((1, 3, 256, 256), generator=g) * 256.0).floor().clamp(max=255.0) for _ in range(K)]
        src_img = [b.to(torch.uint8) if args.compact else b - torch.from_numpy(demo.IMG_MEAN).view(1, 3, 1, 1) for b in src_byte]
        src_lbl, src_box = lbl[:K], box[:K]
    tar_lbl, tar_box, name = lbl[K:], box[K:], args.clip or "synthetic_face"
    if args.drive:
        # the whole driving clip is prepared (the moving average runs over the clip), then the first F frames drive
        t0 = time.perf_counter()
        tar_lbl, tar_box, dcrop, dbw = crossid_labels(rs, kp_all, clip_keypoints(args.drive)[0], compact=args.compact, track_crop=args.track_crop)
        torch.cuda.synchronize()
        F = min(F, tar_lbl.shape[0])
        print(f"[demo_clip] driving labels of {args.drive} adapted to {args.clip}: {tar_lbl.shape[0]} frames (crop {'per frame' if args.track_crop else dcrop}, brush {dbw}) in {(time.perf_counter() - t0) * 1e3:.2f} ms")
        tar_lbl, tar_box, name = tar_lbl[:F], tar_box[:F], f"{args.clip}_by_{args.drive}"
    runner = demo.ClipRunner(model, src_img, [src_lbl[i:i + 1] for i in range(K)], [src_box[i:i + 1] for i in range(K)], batch=args.batch)
    paste = {}
    if args.paste_back:
        fw, fh = tuple(fmeta["frame_size"]) if args.clip else (640, 480)
        min_y, max_y, min_x, max_x = (int(v) for v in crop)
        paste = dict(paste_into=synthetic_frames(F, fh, fw), paste_box=(min_x, min_y, max_x, max_y))
        if args.track_crop:                                      # the driving frames' own crops, (x0, y0, x1, y1)
            pcrops = np.asarray(dcrop if args.drive else tcrops[K:])[:F]
            paste = dict(paste_into=paste["paste_into"], paste_boxes=pcrops[:, [2, 0, 3, 1]])
        print(f"[demo_clip] --paste-back: pasting into SYNTHETIC {fw} x {fh} frames (a gradient; only key points are at hand) at "
              + (f"{F} boxes, one per frame, from {tuple(int(v) for v in paste['paste_boxes'][0])}" if args.track_crop else f"box {paste['paste_box']}"))
    if args.feather is not None:
        paste.update(paste_feather=args.feather, paste_feather_from=args.feather_from or "box")
        print(f"[demo_clip] --feather {args.feather} from {paste['paste_feather_from']}")
    frames = runner.run(tar_lbl, tar_box, out_dir=args.out, name=name, y4m=args.y4m, **paste)
    if args.y4m:
        print(f"[demo_clip] --y4m: {frames.shape[0]} frames of {frames.shape[2]} x {frames.shape[1]} written to {args.y4m}")
    print(f"[demo_clip] {demo.RESIZE_NOTE}")
    print(f"[demo_clip] {frames.shape[0]} {'full ' if args.paste_back else ''}frames written to {args.out} (crop {crop}, brush {bw}); rasterisation of {F + K} frames: {t_raster * 1e3:.2f} ms on the first call; "
          f"steady state " + ", ".join(f"{k} {v * 1e3:.2f} ms" for k, v in t_steps.items()) + f" = {sum(t_steps.values()) / (F + K) * 1e3:.3f} ms per frame")

    # ---- the demo-shaped figure: B = 1, n_blocks = 4, K = 3, clip mode, post-processing included, frames stay on the device
    nb = min(args.batch, F)                                      # driving frames per step: groups of the clip's frames, wrapping around
    steps = (args.timing_frames + nb - 1) // nb
    groups = []                                                  # gathered ahead of the timed loop (the sequence of groups has period <= F)
    for i in range(min(steps, F)):
        j = ((torch.arange(nb) + i * nb) % F).to(dev)
        groups.append((tar_lbl[j], tar_box[j]))
    for _ in range(20):
        runner.frames(*groups[0])
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(steps):
        runner.frames(*groups[i % len(groups)])
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) * args.timing_frames / (steps * nb)
    print(f"[demo_clip] clip mode, B={nb}, n_blocks={args.n_blocks}, K=3: {args.timing_frames / dt:.1f} frames/s ({dt / args.timing_frames * 1e3:.3f} ms per driving frame, "
          "device post-processing included)")


if __name__ == "__main__":
    main()
