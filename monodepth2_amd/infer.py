"""Single-image depth inference (the reference's test_simple.py) on the device.

    python -m monodepth2_amd.infer --image_path FILE_OR_DIR --load_weights_folder DIR \\
        [--ext jpg] [--num_layers 18] [--pred_metric_depth]

For every image this writes, next to the inputs, what the reference writes
(test_simple.py:139-159): NAME_disp.npy, the (1,1,h,w) scaled disparity of
`layers.disp_to_depth(disp, 0.1, 100)` (or NAME_depth.npy, STEREO_SCALE_FACTOR * depth,
with --pred_metric_depth), and NAME_disp.jpeg, the magma picture of the disparity resized
to the original image size.  The networks run through `evaluate_depth.predict_disparities`
(eval mode, no_grad); the picture — resize, 95th percentile, minimum, Normalize, colormap,
uint8, numpy and matplotlib per image on the host in the reference — is the fused HIP
operator of `viz_ops.colorize_disparity`, one call per group of equally sized originals.
NAME_disp.jpeg is encoded on the device from the picture left there (csrc/jpegenc.hip,
quality 75 and 4:2:0, Pillow's defaults): the file is byte-equal to what
`pil.fromarray(picture).save(path)` writes, and no full-size picture is copied to the host.

The feed-size LANCZOS resize and ToTensor (test_simple.py:125-128) run on the device too,
through a one-frame, one-scale `GpuAugment` plan without flip or colour jitter, cached per
input size; a size whose plan cannot be created is resized with PIL on the host instead.

--model_name and its download are deliberately absent: checkpoints come from
--load_weights_folder (encoder.pth with `height` and `width`, depth.pth), read with the
safe loader.
"""
from __future__ import annotations

import argparse
import glob
import os
from typing import Dict, List, Sequence, Tuple

import numpy as np
import PIL.Image as pil
import torch

from . import networks
from .augment import GpuAugment, ItemDraw, pack_items
from .evaluate_depth import STEREO_SCALE_FACTOR, predict_disparities
from .jpeg_ops import encode_jpeg_batch, jpeg_file_bytes
from .layers import disp_to_depth
from .viz_ops import colorize_disparity

BATCH = 16          # images per pass of main()
_plans: Dict[tuple, object] = {}


def load_networks(folder: str, num_layers: int = 18, device="cuda"):
    """(encoder, depth_decoder, (feed_height, feed_width)) of a checkpoint folder
    (test_simple.py:76-100): the feed size is what encoder.pth was trained with."""
    enc_dict = torch.load(os.path.join(folder, "encoder.pth"), map_location=device, weights_only=True)
    if "height" not in enc_dict or "width" not in enc_dict:
        raise SystemExit("{} carries no height / width: not an encoder.pth a training run saved".format(
            os.path.join(folder, "encoder.pth")))
    feed_hw = (int(enc_dict["height"]), int(enc_dict["width"]))
    encoder = networks.ResnetEncoder(num_layers, False)
    model_dict = encoder.state_dict()
    encoder.load_state_dict({k: v for k, v in enc_dict.items() if k in model_dict})
    depth_decoder = networks.DepthDecoder(num_ch_enc=encoder.num_ch_enc, scales=range(4))
    depth_decoder.load_state_dict(torch.load(os.path.join(folder, "depth.pth"), map_location=device,
                                             weights_only=True))
    return encoder.to(device).eval(), depth_decoder.to(device).eval(), feed_hw


def _plan(in_hw: Tuple[int, int], feed_hw: Tuple[int, int], device: torch.device):
    """The cached GpuAugment plan of an input size; None if the library refuses the size."""
    key = (in_hw, feed_hw, device)
    if key not in _plans:
        try:
            _plans[key] = GpuAugment(feed_hw[0], feed_hw[1], in_hw[0], in_hw[1], [0], 1, num_scales=1, device=device)
        except RuntimeError:
            _plans[key] = None
    return _plans[key]


def preprocess(image, feed_hw: Sequence[int], device="cuda") -> torch.Tensor:
    """test_simple.py:125-128: RGB, LANCZOS resize to the feed size, ToTensor -> (1,3,h,w)
    float32 in [0,1] on the device.  `image`: a PIL image or an (H,W,3) uint8 array."""
    device = torch.device(device)
    if device.type == "cuda" and device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    if not isinstance(image, pil.Image):
        image = pil.fromarray(np.asarray(image, dtype=np.uint8))
    image = image.convert("RGB")
    feed_hw = (int(feed_hw[0]), int(feed_hw[1]))
    in_hw = (image.height, image.width)
    plan = _plan(in_hw, feed_hw, device)
    if plan is None:   # PIL on the host
        small = np.array(image.resize((feed_hw[1], feed_hw[0]), pil.LANCZOS), dtype=np.uint8)
        return torch.from_numpy(small).to(device).permute(2, 0, 1).unsqueeze(0).float().div(255).contiguous()
    frames = torch.from_numpy(np.array(image, dtype=np.uint8)).to(device)
    color, _ = plan.run(frames.view(1, 1, in_hw[0], in_hw[1], 3), pack_items([ItemDraw()]))
    return color[0][0]


def _predict(encoder, depth_decoder, images: Sequence, feed_hw: Sequence[int], pred_metric_depth: bool):
    """The shared part of predict_images and predict_files: (PIL images, saved arrays, groups),
    groups a list of (indices, (n, H, W, 3) uint8 device pictures) per original size."""
    if feed_hw[0] % 32 or feed_hw[1] % 32 or min(feed_hw) < 64:
        # the encoder halves five times and the decoder's ReflectionPad2d(1) needs 2 x 2 there
        raise ValueError("the feed size must be a multiple of 32 and at least 64 x 64, got {} x {}".format(*feed_hw))
    device = next(encoder.parameters()).device
    images = [im if isinstance(im, pil.Image) else pil.fromarray(np.asarray(im, dtype=np.uint8)) for im in images]
    x = torch.cat([preprocess(im, feed_hw, device) for im in images])
    disp = predict_disparities(encoder, depth_decoder, x)
    scaled, depth = disp_to_depth(disp, 0.1, 100)
    saved = (STEREO_SCALE_FACTOR * depth if pred_metric_depth else scaled).cpu().numpy()
    groups: Dict[tuple, List[int]] = {}
    for i, im in enumerate(images):
        groups.setdefault((im.height, im.width), []).append(i)
    pictures = []
    for size, idx in groups.items():
        sel = torch.as_tensor(idx, device=device)
        pictures.append((idx, colorize_disparity(disp[sel] if len(idx) != len(images) else disp, size)))
    return images, saved, pictures


def predict_images(encoder, depth_decoder, images: Sequence, feed_hw: Sequence[int],
                   pred_metric_depth: bool = False) -> List[Tuple[np.ndarray, np.ndarray]]:
    """test_simple.py:124-155 for a list of images (PIL images or (H,W,3) uint8 arrays, any
    sizes).  Returns per image (saved, picture): the (1,1,h,w) float32 array the reference
    saves — the scaled disparity, or STEREO_SCALE_FACTOR * depth with `pred_metric_depth` —
    and the (H,W,3) uint8 magma picture at the image's own size.  Images of equal original
    size share one colorize_disparity call; one device-to-host copy per group at the end."""
    if not images:
        return []
    images, saved, groups = _predict(encoder, depth_decoder, images, feed_hw, pred_metric_depth)
    pictures = [None] * len(images)
    for idx, rgb in groups:
        rgb = rgb.cpu().numpy()
        for j, i in enumerate(idx):
            pictures[i] = rgb[j]
    return [(saved[i:i + 1], pictures[i]) for i in range(len(images))]


def predict_files(encoder, depth_decoder, images: Sequence, feed_hw: Sequence[int],
                  pred_metric_depth: bool = False) -> List[Tuple[np.ndarray, bytes]]:
    """predict_images for writing: per image (saved, jpeg), jpeg the bytes of NAME_disp.jpeg.
    The pictures stay where the colour-map chain left them and are encoded there
    (jpeg_ops.encode_jpeg_batch, one call for the whole list) with Pillow's defaults, quality
    75 and 4:2:0; only the compressed streams come back.  Every file is byte-equal to
    `pil.fromarray(picture).save(path)` of predict_images' picture."""
    if not images:
        return []
    images, saved, groups = _predict(encoder, depth_decoder, images, feed_hw, pred_metric_depth)
    order, offsets, sizes, pos = [], [], [], 0
    for idx, rgb in groups:
        n, h, w, _ = rgb.shape
        for j, i in enumerate(idx):
            order.append(i)
            offsets.append(pos + j * h * w * 3)
            sizes.append((h, w))
        pos += n * h * w * 3
    flat = groups[0][1].reshape(-1) if len(groups) == 1 else torch.cat([rgb.reshape(-1) for _, rgb in groups])
    streams = encode_jpeg_batch(flat.contiguous(), quality=75, sampling="4:2:0", device=flat.device, check=True,
                                offsets=offsets, sizes=sizes)
    files = [None] * len(images)
    for i, s in zip(order, streams):
        files[i] = jpeg_file_bytes(s)
    return [(saved[i:i + 1], files[i]) for i in range(len(images))]


def parse_args(argv=None):
    parser = argparse.ArgumentParser(description="Single-image depth inference (the reference's test_simple.py).")
    parser.add_argument("--image_path", type=str, required=True, help="path to a test image or folder of images")
    parser.add_argument("--load_weights_folder", type=str, required=True,
                        help="checkpoint folder with encoder.pth and depth.pth")
    parser.add_argument("--ext", type=str, default="jpg", help="image extension to search for in folder")
    parser.add_argument("--num_layers", type=int, default=18, choices=[18, 34, 50, 101, 152])
    parser.add_argument("--pred_metric_depth", action="store_true",
                        help="if set, predicts metric depth instead of disparity (this only makes sense for "
                             "stereo-trained KITTI models)")
    return parser.parse_args(argv)


def main(argv=None):
    args = parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("monodepth2_amd.infer needs a GPU (HIP kernels, no CPU fallback)")
    device = torch.device("cuda", torch.cuda.current_device())
    folder = os.path.expanduser(args.load_weights_folder)
    if not os.path.isdir(folder):
        raise SystemExit("Cannot find a folder at {}".format(folder))
    print("-> Loading model from ", folder)
    print("   Loading pretrained encoder")
    print("   Loading pretrained decoder")
    encoder, depth_decoder, feed_hw = load_networks(folder, args.num_layers, device)

    if os.path.isfile(args.image_path):
        paths = [args.image_path]
        output_directory = os.path.dirname(args.image_path)
    elif os.path.isdir(args.image_path):
        paths = sorted(glob.glob(os.path.join(args.image_path, "*.{}".format(args.ext))))
        output_directory = args.image_path
    else:
        raise SystemExit("Can not find args.image_path: {}".format(args.image_path))
    print("-> Predicting on {:d} test images".format(len(paths)))

    todo = [(i, p) for i, p in enumerate(paths) if not p.endswith("_disp.jpg")]   # never a picture of a picture
    for start in range(0, len(todo), BATCH):
        chunk = todo[start:start + BATCH]
        results = predict_files(encoder, depth_decoder, [pil.open(p).convert("RGB") for _, p in chunk], feed_hw,
                                args.pred_metric_depth)
        for (idx, path), (saved, picture) in zip(chunk, results):
            name = os.path.splitext(os.path.basename(path))[0]
            npy = os.path.join(output_directory, "{}_{}.npy".format(name, "depth" if args.pred_metric_depth else "disp"))
            np.save(npy, saved)
            jpeg = os.path.join(output_directory, "{}_disp.jpeg".format(name))
            with open(jpeg, "wb") as f:
                f.write(picture)
            print("   Processed {:d} of {:d} images - saved predictions to:".format(idx + 1, len(paths)))
            print("   - {}".format(jpeg))
            print("   - {}".format(npy))
    print("-> Done!")


if __name__ == "__main__":
    main()
