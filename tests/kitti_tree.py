"""A tiny KITTI-raw-shaped tree written with PIL, for the dataset / loader / train tests:
two drives of different native sizes, three consecutive frames each, both cameras."""
import os

import numpy as np
from PIL import Image

DRIVES = [("2011_09_26/2011_09_26_drive_0001_sync", (123, 243)),
          ("2011_09_28/2011_09_28_drive_0002_sync", (121, 240))]
# frame 1 of each drive has both neighbours; drives alternate so a batch of 2 mixes sizes
LINES = ["{} 1 l".format(DRIVES[0][0]), "{} 1 l".format(DRIVES[1][0]),
         "{} 1 r".format(DRIVES[0][0]), "{} 1 r".format(DRIVES[1][0]),
         "{} 1 l".format(DRIVES[0][0])]


def image(rng, h, w):
    """A textured uint8 frame (smooth + noise, like a camera image)."""
    yy, xx = np.mgrid[0:h, 0:w]
    base = np.zeros((h, w, 3))
    for _ in range(5):
        k = rng.uniform(0.02, 0.2, 2)
        base += rng.uniform(20, 60) * np.sin(k[0] * xx + k[1] * yy + rng.uniform(0, 6.3))[..., None] \
            * rng.uniform(0.3, 1.0, 3)
    base += 128 + rng.normal(0, 10, base.shape)
    return np.clip(base, 0, 255).astype(np.uint8)


def write_tree(root, ext=".png", seed=0, depth=False):
    """Writes the tree under `root`; returns {relative path: (h, w, 3) uint8 as written}
    (for PNG that is what decodes; a JPEG is lossy and must be re-opened)."""
    rng = np.random.default_rng(seed)
    written = {}
    for drive, (h, w) in DRIVES:
        for cam in (2, 3):
            folder = os.path.join(root, drive, "image_0{}/data".format(cam))
            os.makedirs(folder, exist_ok=True)
            for frame in range(3):
                arr = image(rng, h, w)
                rel = os.path.join(drive, "image_0{}/data".format(cam), "{:010d}{}".format(frame, ext))
                Image.fromarray(arr).save(os.path.join(root, rel), quality=92) if ext == ".jpg" \
                    else Image.fromarray(arr).save(os.path.join(root, rel))
                written[rel] = arr
        if depth:   # what check_depth looks for, and KITTIDepthDataset's ground truth (16-bit PNG, depth * 256)
            velo = os.path.join(root, drive, "velodyne_points/data")
            os.makedirs(velo, exist_ok=True)
            for frame in range(3):
                open(os.path.join(velo, "{:010d}.bin".format(frame)), "wb").close()
            for cam in (2, 3):
                gt = os.path.join(root, drive, "proj_depth/groundtruth/image_0{}".format(cam))
                os.makedirs(gt, exist_ok=True)
                d = (rng.uniform(0, 80, (h, w)) * 256).astype(np.uint16)
                d[rng.uniform(size=(h, w)) < 0.7] = 0
                Image.fromarray(d).save(os.path.join(gt, "{:010d}.png".format(1)))
    return written


# what KITTIRAWDataset.get_depths reads: per date a calibration whose rectified size is
# KITTI's own (the first 375 x 1242, which needs no resampling, the second one that does)
CALIBRATED = [(375, 1242), (370, 1226)]


def write_velodyne(root, points=20000):
    """Adds calibration files (tests/velo_case.py's synthetic rigs) per date and a scan for
    frame 1 of each drive; returns [(calibration folder, scan file)] in DRIVES order."""
    import velo_case as vc
    frames = []
    for n, ((drive, _), (h, w)) in enumerate(zip(DRIVES, CALIBRATED)):
        calib = vc.write_calib_dir(os.path.join(root, drive.split("/")[0]), vc.calib_texts(h, w, seed=20 + n))
        velo = os.path.join(root, drive, "velodyne_points/data")
        os.makedirs(velo, exist_ok=True)
        scan = os.path.join(velo, "{:010d}.bin".format(1))
        vc.make_scan(points, seed=30 + n).tofile(scan)
        frames.append((calib, scan))
    return frames


def write_splits(folder, train=LINES, val=LINES[:4]):
    os.makedirs(folder, exist_ok=True)
    for name, lines in (("train", train), ("val", val)):
        with open(os.path.join(folder, "{}_files.txt".format(name)), "w") as f:
            f.write("\n".join(lines) + "\n")
    return folder
