"""A tiny KITTI-odometry-shaped tree written with PIL, for the pose evaluation from disk:
six consecutive frames of sequence 09 (camera 2, native size 123 x 243), the six-line
poses/09.txt that goes with them, and the five-line test list (frames k and k + 1)."""
import os

import numpy as np
from PIL import Image

import kitti_tree as KT
import pose_eval_case as pc

SEQUENCE = 9
FRAMES = 6
SIZE = (123, 243)
LINES = ["{} {} l".format(SEQUENCE, k) for k in range(FRAMES - 1)]   # the reference's test_files_09.txt form


def write_tree(root, seed=3):
    """Writes sequences/09/image_2/NNNNNN.png, poses/09.txt and splits/test_files_09.txt
    under `root`; returns the frames as written, [(h, w, 3) uint8] in order."""
    rng = np.random.default_rng(seed)
    folder = os.path.join(root, "sequences", "{:02d}".format(SEQUENCE), "image_2")
    os.makedirs(folder, exist_ok=True)
    frames = []
    for k in range(FRAMES):
        arr = KT.image(rng, *SIZE)
        Image.fromarray(arr).save(os.path.join(folder, "{:06d}.png".format(k)))
        frames.append(arr)
    os.makedirs(os.path.join(root, "poses"), exist_ok=True)
    with open(os.path.join(root, "poses", "{:02d}.txt".format(SEQUENCE)), "w") as f:
        f.write(pc.drive_text(FRAMES, seed=seed))
    os.makedirs(os.path.join(root, "splits"), exist_ok=True)
    with open(os.path.join(root, "splits", "test_files_{:02d}.txt".format(SEQUENCE)), "w") as f:
        f.write("\n".join(LINES) + "\n")
    return frames
