"""`infer` writes NAME_disp.jpeg from the device encoder (csrc/jpegenc.hip): for two images of
different sizes the file is byte-equal to `pil.fromarray(picture).save()` of the picture the
colour-map operator makes of the very disparities that pass produced (recorded by a wrapper:
a second forward pass is not bitwise repeatable, see tests/test_viz_gpu.py)."""
import io

import numpy as np
import pytest
import torch
from PIL import Image

pytestmark = pytest.mark.gpu

FEED = (64, 128)
SIZES = {"a": (37, 50), "b": (40, 71)}


@pytest.fixture(scope="module")
def demo(tmp_path_factory):
    """A random-weight ResNet-18 checkpoint with feed size 64 x 128 and two lossless PNGs of
    different sizes in one folder."""
    from monodepth2_amd import networks
    root = tmp_path_factory.mktemp("infer_jpeg")
    torch.manual_seed(0)
    enc = networks.ResnetEncoder(18, False)
    dec = networks.DepthDecoder(enc.num_ch_enc)
    state = enc.state_dict()
    state["height"], state["width"], state["use_stereo"] = FEED[0], FEED[1], False
    (root / "weights").mkdir()
    torch.save(state, root / "weights" / "encoder.pth")
    torch.save(dec.state_dict(), root / "weights" / "depth.pth")
    (root / "images").mkdir()
    rng = np.random.RandomState(5)
    for i, (name, (h, w)) in enumerate(SIZES.items()):
        yy, xx = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
        img = np.stack([(yy * 5 + xx * 3 + 40 * i) % 256, (xx * 4 + 17) % 256, (yy * 6 + 90 * i) % 256], 2)
        img = np.clip(img + rng.randint(-12, 13, img.shape), 0, 255).astype(np.uint8)
        Image.fromarray(img).save(root / "images" / (name + ".png"))
    return root


def test_disp_jpeg_is_what_pillow_saves(demo, monkeypatch):
    from monodepth2_amd import infer
    from monodepth2_amd.evaluate_depth import predict_disparities
    from monodepth2_amd.viz_ops import colorize_disparity
    calls = []

    def recording(encoder, decoder, x, *args, **kwargs):
        disp = predict_disparities(encoder, decoder, x, *args, **kwargs)
        calls.append(disp.clone())
        return disp

    monkeypatch.setattr(infer, "predict_disparities", recording)
    images = demo / "images"
    infer.main(["--image_path", str(images), "--load_weights_folder", str(demo / "weights"), "--ext", "png"])
    assert len(calls) == 1 and calls[0].shape[0] == 2
    for i, (name, size) in enumerate(SIZES.items()):
        picture = colorize_disparity(calls[0][i:i + 1], size).cpu().numpy()[0]
        assert picture.shape == size + (3,) and picture.dtype == np.uint8
        buf = io.BytesIO()
        Image.fromarray(picture).save(buf, "JPEG")
        got = (images / (name + "_disp.jpeg")).read_bytes()
        assert got == buf.getvalue(), name
        with Image.open(io.BytesIO(got)) as im:
            assert im.size == (size[1], size[0]) and im.mode == "RGB"
