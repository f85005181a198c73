#!/usr/bin/env python3
"""Frame-loop harness with the reference's command line (Testing/test.py:85-107) on the MI355X package.

    python -m tdnet_amd.test --model td4-psp18 --img_path /path/to/frames --output_path ./output/ \\
                             --_td4_psp18_path ./checkpoint/td4-psp18.pkl

Same loop as Testing/test.py:45-81: pos_id = i % path_num, forward timed between two device synchronisations, frames
i > 5 averaged, argmax = output.max(1)[1], quarter-resolution colour PNG per frame.  Differences: PNG I/O through PIL
(imageio / cv2 are not in this image, so no on-screen display); `--gpu` sets HIP_VISIBLE_DEVICES as well;
`--synthetic_seed N` runs on seeded synthetic weights when no checkpoint is available; `--in_size HxW` (default 769x1537,
test.py:24) must match the checkpoint's LayerNorm shape exactly as in the reference; `--u8` keeps the frames as the decoded bytes (the
library resizes and normalises them on the device, bit-identically to the loader) and, with `--prefetch`, is the all-bytes loop: uint8
upload, forward_labels_u8, uint8 label download; `--nv12` turns every frame into an NV12 surface on the host (dataloader.rgb_to_nv12: what a
video decoder would hand over; `--nv12_standard` 0..3) and feeds the surfaces: conversion, resize and normalisation in the frame's first
launch, combinable with `--prefetch`, `--rgb`, `--gt_path` and `--conf` like `--u8`; `--rgb` has the frame's last kernel write the quarter-size colour map itself (the nearest
sample of the label map and decode_segmap, byte for byte): the host downloads the picture and encodes the PNG, nothing else.
`--gt_path DIR` scores the clip against ground truth on the device (single-channel PNGs named like the frames, sampled to `--in_size` with the
nearest rule when their size differs; `--gt_map FILE`: 256 integers as text, ground-truth byte -> class id, anything >= 19 ignored; default
identity): the frame's last kernel counts the confusion matrix, and the four scores and the per-class IoU are printed after the timing block
as Training/validate.py:91-97 prints them.
`--conf DIR` has the frame's last kernel also write the confidence map (the softmax probability of every pixel's label as a byte, 255 = certain) and
saves it at the network size as a grey PNG DIR/folder/name beside the picture; `--min_conf T` (0..1) rejects labels below T: such a pixel gets
label 255 and therefore decode_segmap's grey (255, 255, 255) in the picture.  Either switch selects the frame-by-frame loop's confidence form.
`--overlay ALPHA` (0..1, with `--u8` or `--nv12`) has the frame's last kernel blend the class colours over the frame's own bytes and writes that
SOURCE-size picture instead of the quarter-size colour map (include/tdnet.h "overlay out"); with `--min_conf` the rejected pixels show the bare frame.
`--crop Y,X,H,W` (with `--u8` or `--nv12`) uploads the frames WHOLE and has the device take that rectangle of them in the frame's first launch
(include/tdnet.h "source views"): the result is the one of the pre-cropped frames; with `--overlay` the picture is the rectangle's.
`--yuv LAYOUT` (nv12, nv21, i420, p010, yuy2, uyvy) turns every frame into a tight surface of that layout on the host (dataloader.pack_surface;
`--nv12_standard` 0..3) and feeds the surfaces (include/tdnet.h "surfaces"); it combines with what `--nv12` combines with, `--crop` included.
`--out_yuv LAYOUT:FILE` is `--out_nv12`'s sibling for the destination layouts nv12, nv21, i420 and p010: the device writes every frame's picture through a
destination surface, appended to the raw file.
`--matte IDS` (a comma list of class ids, e.g. 11,12,13,14,15,16,17,18) with `--matte_out DIR` has the frame's last kernel also write the matte -- the
softmax mass of that class set as a byte, 255 = certainly one of them (include/tdnet.h "matte out") -- and saves it at the network size as an 8-bit
grey PNG DIR/folder/name beside the usual picture.  `--matte IDS --composite R,G,B` (with `--u8`, `--nv12` or `--yuv`) writes, where the overlay's
picture would go, the frame seen through the matte over that background, at the frame's own (`--crop`: the rectangle's) size.
`--refine R[,EPS]` with them (and a byte input) guided-filters the matte by the frame's luma (include/tdnet.h "refined matte"): `--matte_out` then writes the
refined matte at the frame's own size (and no label picture), `--composite` composites through it.
`--regions IDS` (a comma list of class ids; `--regions_conn 4|8`, `--regions_min_area N`) labels the connected components of those classes on the device
behind every frame's labels (include/tdnet.h "regions out") and prints the count per frame (`--tracks [MIN_OVERLAP]` follows them across frames, "tracks out":
matched / born / ended per frame, and the columns track,age,origin in the CSVs); `--regions_out DIR` writes one CSV per frame,
DIR/folder/name.csv: id,label,area,x0,y0,x1,y1,cx,cy in network-size pixels.
`--runs [MAX_RUNS]` (fp32 or `--u8` frames) codes every frame's labels as a run-length table on the device behind the label launch (include/tdnet.h
"runs out"); the PNGs are those of the plain loop.  `--runs_out DIR` downloads the tables asynchronously (dataloader.RunsDownloader: the header and the
stored records only) and writes DIR/folder/name.npy: the records (start, value), the closing record last.
"""
import argparse
import os
import timeit

import numpy as np
import torch


def load_ground_truth(gt_path, items, size, nearest_index, pin):
    """One [gt uint8 [1, H, W]] item per frame of `items` ([image, name, folder, size]): the single-channel PNG gt_path/folder/name (or
    gt_path/name), sampled to size = (H, W) with the label map's nearest rule when its size differs."""
    from PIL import Image
    H, W = size
    out = []
    for item in items:
        img_name, folder = item[1], item[2]
        path = os.path.join(gt_path, folder, img_name)
        if not os.path.exists(path):
            path = os.path.join(gt_path, img_name)
        im = Image.open(path)
        if im.mode not in ("L", "P"):
            raise SystemExit("--gt_path: %s is not a single-channel 8-bit PNG (mode %s)" % (path, im.mode))
        g = np.array(im, dtype=np.uint8)
        if g.shape != (H, W):
            g = g[nearest_index(g.shape[0], H)][:, nearest_index(g.shape[1], W)]
        t = torch.from_numpy(np.ascontiguousarray(g)[np.newaxis])
        out.append([t.pin_memory() if pin else t])
    return out


REGIONS_CLI_MAX = 4096                                                 # records of --regions' table: regions beyond are counted, not written


def regions_csv(table, tracks=None):
    """The text --regions_out writes for one frame's records (REGION_DTYPE; record i is region i + 1): id,label,area,x0,y0,x1,y1,cx,cy with the
    centroid sum / area to three decimals.  tracks (--tracks: TRACK_DTYPE, record i for region i + 1) adds the columns track,age,origin."""
    lines = ["id,label,area,x0,y0,x1,y1,cx,cy" + ("" if tracks is None else ",track,age,origin")]
    for i, r in enumerate(table):
        lines.append("%d,%d,%d,%d,%d,%d,%d,%.3f,%.3f" % (i + 1, r["label"], r["area"], r["x0"], r["y0"], r["x1"], r["y1"],
                                                         int(r["sum_x"]) / int(r["area"]), int(r["sum_y"]) / int(r["area"])))
        if tracks is not None:
            lines[-1] += ",%d,%d,%d" % (tracks[i]["track"], tracks[i]["age"], tracks[i]["origin_track"])
    return "\n".join(lines) + "\n"


def yuv_surface(layout, height, width, standard, crop=None):
    """The tight surface --yuv packs a frame into and --out_yuv has the device write: no padding in any row (the chroma rows' own bytes are their pitch)."""
    from tdnet_amd.dataloader import Surface
    t = Surface(layout, height, width)
    return Surface(layout, height, width, chroma_pitch=0 if t.packed422 else t.chroma_row_bytes, crop=crop, standard=standard)


def test(args):
    os.environ["CUDA_VISIBLE_DEVICES"] = args.gpu                      # test.py:19
    os.environ.setdefault("HIP_VISIBLE_DEVICES", args.gpu)
    from tdnet_amd.dataloader import cityscapesLoader, nearest_index
    from tdnet_amd.model import td2_psp50, td4_psp18
    device = torch.device("cuda")
    H, W = (int(v) for v in args.in_size.lower().split("x"))
    u8 = bool(getattr(args, "u8", False))
    nv12 = bool(getattr(args, "nv12", False))
    nv12_std = int(getattr(args, "nv12_standard", 0) or 0)
    yuv = getattr(args, "yuv", None)
    if yuv is not None:                                                # checked before anything is loaded
        from tdnet_amd.dataloader import SURF_NAMES
        if str(yuv).lower() not in SURF_NAMES:
            raise SystemExit("--yuv: one of %s expected, got %r" % (", ".join(sorted(SURF_NAMES)), yuv))
        yuv = SURF_NAMES[str(yuv).lower()]
    if sum((nv12, u8, yuv is not None)) > 1:
        raise SystemExit("--nv12%s and --u8 are two forms of the byte input: choose one" % ("" if yuv is None else ", --yuv"))
    bytes_in = u8 or nv12 or yuv is not None
    crop = getattr(args, "crop", None)
    if crop is not None:                                               # checked before anything is loaded
        if not bytes_in:
            raise SystemExit("--crop takes a rectangle of the frame's own bytes: give --u8 or --nv12 with it")
        try:
            crop = tuple(int(v) for v in str(crop).split(","))
        except ValueError:
            crop = ()
        if len(crop) != 4 or min(crop[:2]) < 0 or min(crop[2:]) < 1:
            raise SystemExit("--crop: Y,X,H,W expected (the rectangle's origin and size in frame pixels), got %r" % (args.crop,))
    rgb = bool(getattr(args, "rgb", False))
    overlay = getattr(args, "overlay", None)
    if overlay is not None:                                            # checked before anything is loaded
        if not bytes_in:
            raise SystemExit("--overlay blends the class colours over the frame's own bytes: give --u8 or --nv12 with it (an fp32 tensor has no source bytes)")
        if rgb or getattr(args, "gt_path", None):
            raise SystemExit("--overlay, --rgb and --gt_path ask for different last kernels: choose one")
        if not 0.0 <= overlay <= 1.0:
            raise SystemExit("--overlay: an opacity in 0..1 expected, got %r" % (overlay,))
    matte_ids, matte_dir, composite = getattr(args, "matte", None), getattr(args, "matte_out", None), getattr(args, "composite", None)
    if matte_ids is not None or matte_dir is not None or composite is not None:   # checked before anything is loaded
        if matte_ids is None:
            raise SystemExit("--matte_out and --composite need the class set: give --matte IDS (a comma list of class ids) with them")
        try:
            matte_ids = tuple(int(v) for v in str(matte_ids).split(",") if v.strip() != "")
        except ValueError:
            matte_ids = (-1,)
        if any(c < 0 or c >= 19 for c in matte_ids):
            raise SystemExit("--matte: a comma list of class ids in 0..18 expected, got %r" % (args.matte,))
        if (matte_dir is None) == (composite is None):
            raise SystemExit("--matte selects the frame's last kernel: give --matte_out DIR (the matte as a PNG) or --composite R,G,B (the frame through it), one of them")
        if rgb or overlay is not None or getattr(args, "gt_path", None) or getattr(args, "prefetch", False) or getattr(args, "conf", None) is not None or \
                getattr(args, "min_conf", None) is not None or getattr(args, "out_nv12", None) is not None or getattr(args, "out_yuv", None) is not None:
            raise SystemExit("--matte asks for a last kernel of its own in the frame-by-frame loop: not with --rgb, --overlay, --gt_path, --prefetch, --conf, --min_conf, "
                             "--out_nv12 or --out_yuv")
        if composite is not None:
            if not bytes_in:
                raise SystemExit("--composite cuts the frame's own bytes out: give --u8, --nv12 or --yuv with it (an fp32 tensor has no source bytes)")
            try:
                composite = tuple(int(v) for v in str(composite).split(","))
            except ValueError:
                composite = ()
            if len(composite) != 3 or any(v < 0 or v > 255 for v in composite):
                raise SystemExit("--composite: R,G,B expected (the background, three byte values), got %r" % (args.composite,))
    with_matte = matte_ids is not None
    refine = getattr(args, "refine", None)
    if refine is not None:                                             # checked before anything is loaded
        if not with_matte:
            raise SystemExit("--refine filters the matte: give --matte IDS with --matte_out DIR or --composite R,G,B with it")
        if not bytes_in:
            raise SystemExit("--refine takes the frame's own luma as its guide: give --u8, --nv12 or --yuv with it (an fp32 tensor has no source bytes)")
        try:
            refine = tuple(int(v) for v in str(refine).split(","))
        except ValueError:
            refine = ()
        if len(refine) == 1:
            refine = refine + (65,)
        if len(refine) != 2 or not 1 <= refine[0] <= 16 or not 4 <= refine[1] <= 65025:
            raise SystemExit("--refine: R[,EPS] expected, a radius in 1..16 and eps in 4..65025 (squared byte units, default 65), got %r" % (args.refine,))
    region_ids, regions_dir = getattr(args, "regions", None), getattr(args, "regions_out", None)
    regions_conn, regions_min_area = getattr(args, "regions_conn", None), getattr(args, "regions_min_area", None)
    if region_ids is not None or regions_dir is not None or regions_conn is not None or regions_min_area is not None:   # checked before anything is loaded
        if region_ids is None:
            raise SystemExit("--regions_conn, --regions_min_area and --regions_out need the class set: give --regions IDS (a comma list of class ids) with them")
        try:
            region_ids = tuple(int(v) for v in str(region_ids).split(",") if v.strip() != "")
        except ValueError:
            region_ids = (-1,)
        if any(c < 0 or c >= 19 for c in region_ids):
            raise SystemExit("--regions: a comma list of class ids in 0..18 expected, got %r" % (args.regions,))
        regions_conn = 8 if regions_conn is None else regions_conn
        regions_min_area = 1 if regions_min_area is None else regions_min_area
        if regions_conn not in (4, 8) or regions_min_area < 1:
            raise SystemExit("--regions_conn: 4 or 8 expected, --regions_min_area: at least 1; got %r and %r" % (regions_conn, regions_min_area))
        if rgb or overlay is not None or with_matte or getattr(args, "gt_path", None) or getattr(args, "prefetch", False) or getattr(args, "conf", None) is not None or \
                getattr(args, "min_conf", None) is not None or getattr(args, "out_nv12", None) is not None or getattr(args, "out_yuv", None) is not None:
            raise SystemExit("--regions asks for a tail of its own in the frame-by-frame loop: not with --rgb, --overlay, --matte, --gt_path, --prefetch, --conf, --min_conf, "
                             "--out_nv12 or --out_yuv")
    with_regions = region_ids is not None
    min_overlap = getattr(args, "tracks", None)                        # --tracks [MIN_OVERLAP]: checked before anything is loaded
    if min_overlap is not None and not with_regions:
        raise SystemExit("--tracks follows the regions of --regions across frames: give --regions IDS (a comma list of class ids) with it")
    if min_overlap is not None and min_overlap < 1:
        raise SystemExit("--tracks: a minimum overlap of at least 1 pixel expected, got %r" % (min_overlap,))
    with_tracks = min_overlap is not None
    max_runs, runs_dir = getattr(args, "runs", None), getattr(args, "runs_out", None)   # --runs [MAX_RUNS]: checked before anything is loaded
    if runs_dir is not None and max_runs is None:
        raise SystemExit("--runs_out writes the tables of --runs: give --runs [MAX_RUNS] with it")
    if max_runs is not None:
        if max_runs != 0 and not 1 <= max_runs <= H * W:
            raise SystemExit("--runs: a table of 1 .. %d runs (H W) expected, got %r" % (H * W, max_runs))
        if rgb or overlay is not None or with_matte or with_regions or getattr(args, "gt_path", None) or getattr(args, "prefetch", False) or \
                getattr(args, "conf", None) is not None or getattr(args, "min_conf", None) is not None or nv12 or crop is not None or yuv is not None or \
                getattr(args, "out_nv12", None) is not None or getattr(args, "out_yuv", None) is not None:
            raise SystemExit("--runs asks for a tail of its own in the frame-by-frame loop: with --u8 or fp32 frames only, not with --rgb, --overlay, --matte, --regions, "
                             "--gt_path, --prefetch, --conf, --min_conf, --nv12, --yuv, --crop, --out_nv12 or --out_yuv")
    with_runs = max_runs is not None
    out_nv12, out_yuv = getattr(args, "out_nv12", None), getattr(args, "out_yuv", None)
    out_layout = None
    if out_yuv is not None:                                            # LAYOUT:FILE; checked before anything is loaded
        from tdnet_amd.dataloader import SURF_DST, SURF_NAMES
        name, _, path = str(out_yuv).partition(":")
        if SURF_NAMES.get(name.lower()) not in SURF_DST or not path:
            raise SystemExit("--out_yuv: LAYOUT:FILE expected with LAYOUT one of nv12, nv21, i420, p010 (no encoder takes yuy2 / uyvy), got %r" % (out_yuv,))
        if out_nv12 is not None:
            raise SystemExit("--out_yuv and --out_nv12 name the same raw file two ways: choose one")
        out_layout, out_nv12 = SURF_NAMES[name.lower()], path
    if out_nv12 is not None:                                           # checked before anything is loaded
        if not bytes_in or not (rgb or overlay is not None):
            raise SystemExit("--out_nv12 writes the frame's picture as NV12 surfaces: give --rgb or --overlay, and --u8 or --nv12, with it")
        if getattr(args, "prefetch", False) or getattr(args, "gt_path", None) or getattr(args, "conf", None) is not None or getattr(args, "min_conf", None) is not None:
            raise SystemExit("--out_nv12 belongs to the frame-by-frame picture loop: not with --prefetch, --gt_path, --conf or --min_conf")
    vid_seq = cityscapesLoader(img_path=args.img_path, in_size=(H, W), pin_memory=getattr(args, "prefetch", False), as_uint8=u8 or yuv is not None, as_nv12=nv12,
                               nv12_standard=nv12_std)
    vid_seq.load_frames()
    if yuv is not None:                                                # every frame a tight surface [1, nbytes]; the item carries (Hs, Ws) like an NV12 item
        from tdnet_amd.dataloader import pack_surface
        for item in vid_seq.data:
            frame = item[0][0].numpy()
            t = torch.from_numpy(pack_surface(frame, yuv_surface(yuv, frame.shape[0], frame.shape[1], nv12_std))[np.newaxis])
            item[0] = t.pin_memory() if getattr(args, "prefetch", False) else t
            item.append((frame.shape[0], frame.shape[1]))
    if args.model == "td4-psp18":
        path_num = 4
        model = td4_psp18.td4_psp18(nclass=19, path_num=path_num, model_path=args._td4_psp18_path, synthetic_seed=args.synthetic_seed)
    elif args.model in ("td2-psp50", "td2-psp18", "td2-psp34"):
        path_num = 2
        model = td2_psp50.td2_psp50(nclass=19, path_num=path_num, model_path=args._td2_psp50_path,
                                    backbone="resnet" + args.model[-2:], synthetic_seed=args.synthetic_seed)
    elif args.model == "psp101":                                        # test.py:34-38
        path_num = 1
        from tdnet_amd.model import pspnet
        model = pspnet.pspnet(nclass=19, model_path=args._psp101_path, synthetic_seed=args.synthetic_seed)
    else:
        raise SystemExit("model must be one of td4-psp18, td2-psp50, td2-psp18, td2-psp34, psp101")
    model.eval()
    model.to(device)
    gts, gt_map = None, None
    if getattr(args, "gt_path", None):
        if rgb:
            raise SystemExit("--gt_path and --rgb ask for two different last kernels: choose one")
        gts = load_ground_truth(args.gt_path, vid_seq.data, (H, W), nearest_index, getattr(args, "prefetch", False))
        if getattr(args, "gt_map", None):
            gt_map = np.array(open(args.gt_map).read().split(), dtype=np.int64)
            if gt_map.shape != (256,) or gt_map.min() < 0 or gt_map.max() > 255:
                raise SystemExit("--gt_map: 256 integers in 0..255 expected, got %d" % gt_map.size)
            gt_map = gt_map.astype(np.uint8)

    conf_dir, min_conf = getattr(args, "conf", None), getattr(args, "min_conf", None)
    with_conf = conf_dir is not None or min_conf is not None
    if with_conf:
        if rgb or gts is not None or getattr(args, "prefetch", False):
            raise SystemExit("--conf / --min_conf select the frame's last kernel of the frame-by-frame loop: not with --rgb, --gt_path or --prefetch")
        if min_conf is not None and not 0.0 <= min_conf <= 1.0:
            raise SystemExit("--min_conf: a probability in 0..1 expected, got %r" % (min_conf,))
        model.set_confidence(min_conf or 0.0, 255)

    if with_matte:
        model.set_matte(matte_ids)
    if refine is not None:
        model.set_matte_refine(*refine)
    if with_regions:
        model.set_regions(region_ids, regions_conn, REGIONS_CLI_MAX, regions_min_area)
    if with_tracks:
        model.set_tracks(min_overlap)
    runs_down = None
    if with_runs:
        from tdnet_amd.dataloader import RunsDownloader
        model.set_runs(max_runs or None)                               # --runs without a value: H W, every map fits
        runs_down = RunsDownloader(device)

    def save_runs(arrived):                                            # --runs_out: one .npy of records (start, value; the closing record last) per frame
        for (img_name, folder), hdr, recs in arrived:
            if runs_dir is not None:
                os.makedirs(os.path.join(runs_dir, folder), exist_ok=True)
                np.save(os.path.join(runs_dir, folder, os.path.splitext(img_name)[0] + ".npy"), recs)

    def save_regions(table, img_name, folder, tracks=None):            # --regions_out: one CSV per frame; the centroid is sum / area
        os.makedirs(os.path.join(regions_dir, folder), exist_ok=True)
        with open(os.path.join(regions_dir, folder, os.path.splitext(img_name)[0] + ".csv"), "w") as f:
            f.write(regions_csv(table, tracks))

    def print_scores():                                                # Training/validate.py:91-97
        if gts is None:
            return
        score, class_iou = model.get_scores()
        for k, v in score.items():
            print(k, v)
        for c in range(model.nclass):
            print(c, class_iou[c])

    def write_png(picture, img_name, folder):
        save_dir = os.path.join(args.output_path, folder)
        os.makedirs(save_dir, exist_ok=True)
        from PIL import Image
        Image.fromarray(picture).save(os.path.join(save_dir, img_name))

    def save(pred, img_name, folder, ori_size):
        pred = np.squeeze(pred, axis=0).astype(np.int8)
        # cv2.resize(pred, (W//4, H//4), INTER_NEAREST) (test.py:64): nearest sample at floor(dst * scale)
        ys, xs = nearest_index(pred.shape[0], ori_size[1] // 4), nearest_index(pred.shape[1], ori_size[0] // 4)
        write_png(vid_seq.decode_segmap(pred[ys][:, xs]).astype(np.uint8), img_name, folder)

    def save_conf(pred, conf, img_name, folder, ori_size):             # --conf / --min_conf: uint8 labels (255 = rejected -> grey) and the confidence map
        pred = np.squeeze(pred, axis=0).astype(np.int16)
        ys, xs = nearest_index(pred.shape[0], ori_size[1] // 4), nearest_index(pred.shape[1], ori_size[0] // 4)
        write_png(vid_seq.decode_segmap(pred[ys][:, xs]).astype(np.uint8), img_name, folder)
        if conf_dir is not None:
            os.makedirs(os.path.join(conf_dir, folder), exist_ok=True)
            from PIL import Image
            Image.fromarray(np.squeeze(conf, axis=0)).save(os.path.join(conf_dir, folder, img_name))

    def save_matte(pred, matte, img_name, folder, ori_size):           # --matte_out: the usual picture of the uint8 labels, and the matte at the network size
        save(pred, img_name, folder, ori_size)
        os.makedirs(os.path.join(matte_dir, folder), exist_ok=True)
        from PIL import Image
        Image.fromarray(np.squeeze(matte, axis=0)).save(os.path.join(matte_dir, folder, img_name))

    def save_rgb(picture, img_name, folder, ori_size):                 # --rgb: the device wrote the picture
        write_png(np.squeeze(picture, axis=0), img_name, folder)

    def through_view(image, src_size):
        """--crop: the WHOLE frame as bytes [1, nbytes] and the view that takes the rectangle of it (the frame is uploaded as it is; the byte
        methods read the rectangle in the frame's first launch, the overlay in its last)."""
        from tdnet_amd.dataloader import PIX_NV12, PIX_RGB24, SourceView
        if yuv is not None:
            return image.reshape(1, -1), yuv_surface(yuv, src_size[0], src_size[1], nv12_std, crop)
        if nv12:
            v = SourceView(PIX_NV12, src_size[0], src_size[1], pitch=int(image.shape[2]), crop=crop, standard=nv12_std)
        else:
            v = SourceView(PIX_RGB24, int(image.shape[1]), int(image.shape[2]), crop=crop)
        return image.reshape(1, -1), v

    as_view = crop is not None or (nv12 and (with_matte or with_regions))   # --matte, --regions: an NV12 surface goes through the byte methods as the whole NV12 view (through_view with no crop)
    nvp, byte = nv12 and not as_view, u8 or as_view or yuv is not None   # with --crop an NV12 surface goes through the byte methods too, as an NV12 view
    described = as_view or yuv is not None                             # the frame goes up WHOLE with a description: a source view, or (--yuv) a surface

    def vk(v):
        return {"surface": v} if yuv is not None else {"view": v}

    def colour_map(image, pos_id, ori_size, src_size=None, view=None):   # [1, oh, ow, 3] uint8 on the device
        out_size = (ori_size[1] // 4, ori_size[0] // 4)
        if nvp:
            return model.forward_rgb_nv12(image, pos_id, src_size, (H, W), out_size, standard=nv12_std)
        if byte:
            return model.forward_rgb_u8(image, pos_id, (H, W), out_size, **vk(view))
        return model.forward_rgb(image, pos_id, out_size)

    def overlay_picture(image, pos_id, src_size=None, view=None):      # --overlay: [1, Hs, Ws, 3] uint8 on the device, at the source's (--crop: the rectangle's) size
        if nvp:
            return model.forward_overlay_nv12(image, pos_id, src_size, (H, W), alpha=overlay, standard=nv12_std)
        return model.forward_overlay_u8(image, pos_id, (H, W), alpha=overlay, **vk(view))

    raw_files = {}

    def pictures_nv12(l8, image, ori_size, src_size, view, folder):
        """--out_nv12: the picture of the frame's uint8 labels twice, by the unfused entries -- contiguous RGB for the PNG (byte for byte the fused entry's)
        and through an NV12 destination view, the whole tight surface, appended to the clip's raw file (what `-f rawvideo -pix_fmt nv12` reads)."""
        from tdnet_amd.dataloader import PIX_NV12, SourceView
        if rgb:
            size = (ori_size[1] // 4, ori_size[0] // 4)
            draw = lambda **kw: model.labels_rgb(l8, size, **kw)
        else:
            draw = lambda **kw: model.labels_overlay(l8, image, alpha=overlay, src_size=src_size if nvp else None, standard=nv12_std, **vk(view), **kw)
        picture = draw()
        if out_layout is not None:                                     # --out_yuv: a destination surface
            surf = draw(out_surface=yuv_surface(out_layout, int(picture.shape[1]), int(picture.shape[2]), nv12_std))
        else:
            surf = draw(out_view=SourceView(PIX_NV12, int(picture.shape[1]), int(picture.shape[2]), standard=nv12_std))
        if folder not in raw_files:                                    # one raw file per clip: the first clip's is FILE itself
            root, ext = os.path.splitext(out_nv12)
            raw_files[folder] = out_nv12 if not raw_files else root + "." + folder + ext
            open(raw_files[folder], "wb").close()
        with open(raw_files[folder], "ab") as f:
            f.write(surf[0].cpu().numpy().tobytes())
        return picture

    timer, i = 0.0, -1
    with torch.no_grad():
        if args.prefetch:
            # throughput loop (not in the reference): frame i + 1 is uploaded while frame i computes, the labels come back
            # asynchronously as int32 (the full-resolution logits are never written), PNGs are written as they arrive
            from tdnet_amd.dataloader import DevicePrefetcher, LabelDownloader
            down = LabelDownloader(device)
            torch.cuda.synchronize()
            start_time = timeit.default_timer()
            gt_feed = iter(DevicePrefetcher(gts, device)) if gts is not None else None   # the ground truth travels with the frame
            for i, (image, img_name, folder, ori_size, *rest) in enumerate(DevicePrefetcher(vid_seq.data, device)):
                src_size = rest[0] if nv12 or yuv is not None else None   # an NV12 / --yuv item carries the picture's (Hs, Ws)
                view = None
                if described:
                    image, view = through_view(image, src_size)
                if gt_feed is not None:
                    gt = next(gt_feed)[0]
                    if nvp:
                        labels = model.forward_score_nv12(image, gt, i % path_num, src_size, (H, W), gt_map=gt_map, return_labels=True, standard=nv12_std)
                    elif byte:
                        labels = model.forward_score_u8(image, gt, i % path_num, (H, W), gt_map=gt_map, return_labels=True, **vk(view))
                    else:
                        labels = model.forward_score(image, gt, i % path_num, gt_map=gt_map, return_labels=True)
                elif rgb:
                    labels = colour_map(image, i % path_num, ori_size, src_size, view)
                elif overlay is not None:
                    labels = overlay_picture(image, i % path_num, src_size, view)
                elif nvp:
                    labels = model.forward_labels_nv12(image, i % path_num, src_size, (H, W), standard=nv12_std)
                else:
                    labels = model.forward_labels_u8(image, pos_id=i % path_num, in_size=(H, W), **vk(view)) if byte else model.forward_labels(image, pos_id=i % path_num)
                for tag, pred in down.submit(labels, (img_name, folder, ori_size)):
                    (save_rgb if rgb or overlay is not None else save)(pred, *tag)
            for tag, pred in down.drain():
                (save_rgb if rgb or overlay is not None else save)(pred, *tag)
            torch.cuda.synchronize()
            timer = timeit.default_timer() - start_time
            print("---------------------")
            print(" Model: {0:s}".format(args.model))
            if i >= 0:
                print(" {0:d} frames, prefetched upload + asynchronous labels: {1:3.5f} s per frame including the PNG writer".format(i + 1, timer / (i + 1)))
            print("---------------------")
            print_scores()
            return
        for i, (image, img_name, folder, ori_size, *rest) in enumerate(vid_seq.data):
            src_size = rest[0] if nv12 or yuv is not None else None
            image = image.to(device)
            view = None
            if described:
                image, view = through_view(image, src_size)
            gt = gts[i][0].to(device) if gts is not None else None
            torch.cuda.synchronize()
            start_time = timeit.default_timer()
            if gt is not None and nvp:
                output = model.forward_score_nv12(image, gt, i % path_num, src_size, (H, W), gt_map=gt_map, return_labels=True, standard=nv12_std)
            elif gt is not None and byte:
                output = model.forward_score_u8(image, gt, i % path_num, (H, W), gt_map=gt_map, return_labels=True, **vk(view))
            elif gt is not None:
                output = model.forward_score(image, gt, i % path_num, gt_map=gt_map, return_labels=True)
            elif out_nv12 is not None:
                l8 = model.forward_labels_nv12(image, i % path_num, src_size, (H, W), standard=nv12_std) if nvp else \
                    model.forward_labels_u8(image, i % path_num, (H, W), **vk(view))
                output = pictures_nv12(l8, image, ori_size, src_size, view, folder)
            elif composite is not None:
                output = model.forward_composite_u8(image, i % path_num, (H, W), background=composite, **vk(view))
            elif with_matte and refine is not None:                    # --matte_out with --refine: the refined matte at the frame's own size, no label picture
                matte = model.forward_matte_refined_u8(image, i % path_num, (H, W), **vk(view))
                output = None
            elif with_matte:
                output, matte = model.forward_matte_u8(image, i % path_num, (H, W), **vk(view)) if byte else model.forward_matte(image, i % path_num)
            elif with_tracks:
                output, _, tables, _, tracks = model.forward_tracks_u8(image, i % path_num, (H, W), return_ids=False, return_track_ids=False, **vk(view)) if byte else \
                    model.forward_tracks(image, i % path_num, return_ids=False, return_track_ids=False)
            elif with_regions:
                output, _, tables = model.forward_regions_u8(image, i % path_num, (H, W), return_ids=False, **vk(view)) if byte else \
                    model.forward_regions(image, i % path_num, return_ids=False)
            elif with_runs:
                output, rtable, _ = model.forward_u8_runs(image, i % path_num, (H, W)) if byte else model.forward_runs(image, i % path_num)
            elif rgb:
                output = colour_map(image, i % path_num, ori_size, src_size, view)
            elif overlay is not None and with_conf:                    # the accepted pixels tinted, the rejected ones (label 255) the bare frame
                if nvp:
                    l8, conf = model.forward_labels_conf_nv12(image, i % path_num, src_size, (H, W), standard=nv12_std)
                else:
                    l8, conf = model.forward_labels_conf_u8(image, i % path_num, (H, W), **vk(view))
                output = model.labels_overlay(l8, image, alpha=overlay, src_size=src_size if nvp else None, standard=nv12_std, **vk(view))
            elif overlay is not None:
                output = overlay_picture(image, i % path_num, src_size, view)
            elif with_conf and nvp:
                output, conf = model.forward_labels_conf_nv12(image, i % path_num, src_size, (H, W), standard=nv12_std)
            elif nvp:
                output = model.forward_nv12(image, i % path_num, src_size, (H, W), standard=nv12_std)
            elif with_conf:
                output, conf = model.forward_labels_conf_u8(image, i % path_num, (H, W), **vk(view)) if byte else model.forward_labels_conf(image, i % path_num)
            else:
                output = model.forward_u8(image, pos_id=i % path_num, in_size=(H, W), **vk(view)) if byte else model(image, pos_id=i % path_num)
            torch.cuda.synchronize()
            elapsed_time = timeit.default_timer() - start_time
            if i > 5:
                timer += elapsed_time
            if gt is not None:
                save(output.cpu().numpy(), img_name, folder, ori_size)
            elif with_matte and composite is None and refine is not None:
                os.makedirs(os.path.join(matte_dir, folder), exist_ok=True)
                from PIL import Image
                Image.fromarray(np.squeeze(matte.cpu().numpy(), axis=0)).save(os.path.join(matte_dir, folder, img_name))
            elif with_matte and composite is None:
                save_matte(output.cpu().numpy(), matte.cpu().numpy(), img_name, folder, ori_size)
            elif with_regions:                                         # the usual picture of the uint8 labels, and the frame's regions
                save(output.cpu().numpy(), img_name, folder, ori_size)
                print(" Frame {0:2d}   {1:d} regions{2:s}{3:s}".format(
                    i + 1, tables[0].count, "" if tables[0].count == len(tables[0]) else " (%d in the table)" % len(tables[0]),
                    "" if not with_tracks else "   matched / born / ended {0:d} / {1:d} / {2:d}".format(tracks[0].matched, len(tracks[0]) - tracks[0].matched, tracks[0].ended)))
                if regions_dir is not None:
                    save_regions(tables[0], img_name, folder, tracks[0] if with_tracks else None)
            elif with_runs:                                            # the usual picture of the uint8 labels; the table travels beside it
                save(output.cpu().numpy(), img_name, folder, ori_size)
                save_runs(runs_down.submit(rtable[0], (img_name, folder)))
            elif rgb or overlay is not None or composite is not None:
                save_rgb(output.cpu().numpy(), img_name, folder, ori_size)
                if overlay is not None and conf_dir is not None:
                    os.makedirs(os.path.join(conf_dir, folder), exist_ok=True)
                    from PIL import Image
                    Image.fromarray(np.squeeze(conf.cpu().numpy(), axis=0)).save(os.path.join(conf_dir, folder, img_name))
            elif with_conf:
                save_conf(output.cpu().numpy(), conf.cpu().numpy(), img_name, folder, ori_size)
            else:
                save(output.data.max(1)[1].cpu().numpy(), img_name, folder, ori_size)
            print(" Frame {0:2d}   RunningTime/Latency={1:3.5f} s".format(i + 1, elapsed_time))
    if runs_down is not None:
        save_runs(runs_down.drain())
    print("---------------------")
    print(" Model: {0:s}".format(args.model))
    if i > 5:
        print(" Average  RunningTime/Latency={0:3.5f} s".format(timer / (i - 5)))
    print("---------------------")
    print_scores()


if __name__ == "__main__":
    parser = argparse.ArgumentParser(description="Params")
    parser.add_argument("--img_path", nargs="?", type=str, default="./data/vid1", help="Path_to_Frame")
    parser.add_argument("--output_path", nargs="?", type=str, default="./output/", help="Path_to_Save")
    parser.add_argument("--_td4_psp18_path", nargs="?", type=str, default="./checkpoint/td4-psp18.pkl", help="Path_to_PSP_Model")
    parser.add_argument("--_td2_psp50_path", nargs="?", type=str, default="./checkpoint/td2-psp50.pkl", help="Path_to_PSP_Model")
    parser.add_argument("--_psp101_path", nargs="?", type=str, default="./checkpoint/psp101.pkl", help="Path_to_PSP_Model")
    parser.add_argument("--gpu", nargs="?", type=str, default="0", help="gpu_id")
    parser.add_argument("--model", nargs="?", type=str, default="td4-psp18", help="model in [td4-psp18, td2-psp50, td2-psp18, td2-psp34]")
    parser.add_argument("--in_size", nargs="?", type=str, default="769x1537", help="HxW fed to the network (test.py:24)")
    parser.add_argument("--synthetic_seed", nargs="?", type=int, default=None, help="run on seeded synthetic weights")
    parser.add_argument("--prefetch", action="store_true", help="throughput loop: upload of the next frame under the current one, asynchronous label download")
    parser.add_argument("--u8", action="store_true", help="frames stay uint8 HWC at their source size: resize + normalisation on the device (bit-identical); with --prefetch uint8 labels too")
    parser.add_argument("--nv12", action="store_true", help="frames go to the device as NV12 surfaces (Y plane + interleaved UV plane, padded pitch): colour conversion, resize and normalisation in the frame's first launch")
    parser.add_argument("--nv12_standard", nargs="?", type=int, default=0, help="the surfaces' YUV standard: 0 BT.601 limited (default), 1 BT.709 limited, 2 BT.601 full, 3 BT.709 full")
    parser.add_argument("--rgb", action="store_true", help="the frame's last kernel writes the quarter-size colour map: no label download, resize or decode_segmap on the host")
    parser.add_argument("--gt_path", nargs="?", type=str, default=None, help="ground-truth PNGs (single channel, named like the frames): score the clip on the device and print the scores")
    parser.add_argument("--gt_map", nargs="?", type=str, default=None, help="text file of 256 integers: ground-truth byte -> class id (>= 19: ignored); default identity")
    parser.add_argument("--conf", nargs="?", type=str, default=None, help="directory for each frame's confidence map (grey PNG at the network size; 255 = certain)")
    parser.add_argument("--min_conf", nargs="?", type=float, default=None, help="reject labels whose softmax probability is below this (0..1): label 255, grey in the picture")
    parser.add_argument("--matte", nargs="?", type=str, default=None, help="comma list of class ids (e.g. 11,12,13,14,15,16,17,18): the class set of --matte_out / --composite")
    parser.add_argument("--matte_out", nargs="?", type=str, default=None, help="with --matte: directory for each frame's matte (8-bit grey PNG at the network size; 255 = certainly a member of the set)")
    parser.add_argument("--refine", nargs="?", type=str, default=None, help="with --matte and --u8, --nv12 or --yuv: R[,EPS] -- guided-filter the matte by the frame's luma (radius 1..16, eps 4..65025 in squared byte units, default 65): --matte_out then writes the refined matte at the frame's own size, --composite uses it")
    parser.add_argument("--composite", nargs="?", type=str, default=None, help="with --matte and --u8, --nv12 or --yuv: R,G,B -- write the frame seen through the matte over this background, at the frame's own size, where the overlay's picture would go")
    parser.add_argument("--regions", nargs="?", type=str, default=None, help="comma list of class ids (e.g. 11,12,13): label the connected components of these classes on the device behind every frame's labels")
    parser.add_argument("--regions_conn", nargs="?", type=int, default=None, help="with --regions: 4 or 8 neighbours (default 8)")
    parser.add_argument("--regions_min_area", nargs="?", type=int, default=None, help="with --regions: drop regions of fewer pixels (default 1)")
    parser.add_argument("--tracks", nargs="?", type=int, const=1, default=None, help="with --regions: follow the regions across frames on the device (optional value: the minimum overlap in pixels of a match, default 1); prints matched / born / ended per frame, --regions_out CSVs gain track,age,origin")
    parser.add_argument("--regions_out", nargs="?", type=str, default=None, help="with --regions: directory for one CSV per frame: id,label,area,x0,y0,x1,y1,cx,cy (network-size pixels, inclusive box)")
    parser.add_argument("--runs", nargs="?", type=int, const=0, default=None, help="code every frame's labels as a run-length table on the device behind the label launch (optional value: the runs a table holds, default H W: every map fits); the PNGs are those of the plain loop")
    parser.add_argument("--runs_out", nargs="?", type=str, default=None, help="with --runs: directory for one .npy per frame: the records (start, value) of the frame's runs and the closing record, downloaded asynchronously")
    parser.add_argument("--overlay", nargs="?", type=float, default=None, help="with --u8 or --nv12: write the class colours blended over the frame at this opacity (0..1), at the frame's own size")
    parser.add_argument("--out_nv12", nargs="?", type=str, default=None, help="with --rgb or --overlay (and --u8 or --nv12): append every frame's picture as a tight NV12 surface (--nv12_standard) to this raw file, written by the device through a destination view; a further clip's surfaces go to FILE with the clip's folder name in front of the extension")
    parser.add_argument("--yuv", nargs="?", type=str, default=None, help="frames go to the device as tight surfaces of this layout (nv12, nv21, i420, p010, yuy2, uyvy; --nv12_standard): conversion, resize and normalisation in the frame's first launch; combines with what --nv12 combines with, --crop included")
    parser.add_argument("--out_yuv", nargs="?", type=str, default=None, help="LAYOUT:FILE -- --out_nv12's sibling for nv12, nv21, i420 and p010: every frame's picture appended to FILE as a tight surface of that layout, written by the device through a destination surface")
    parser.add_argument("--crop", nargs="?", type=str, default=None, help="with --u8 or --nv12: Y,X,H,W -- the frames are uploaded whole and the rectangle is taken on the device, in the frame's first launch (a source view)")
    test(parser.parse_args())
