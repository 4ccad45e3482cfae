"""The yardstick of md2_log_panel: a numpy restatement, in the operator's stated order and in
fp32, of the quantisation, the per-map statistics, normalize_image (reference utils.py:22-28)
and the tile placement of the training log's contact sheet.  No torch.

tests/golden/logpanel/make_logpanel_golden.py pins `normalize` to the reference's own
normalize_image on the CPU, bit for bit, on `disp_cases()`.
"""
import numpy as np

COLOR, WARP, DISP, MAP = 0, 1, 2, 3
F255 = np.float32(255.0)


def quantise(x):
    """uint8(clip(fp32(x) * fp32(255), 0, 255)): one fp32 product, truncation; NaN gives 0."""
    with np.errstate(invalid="ignore", over="ignore"):
        p = np.asarray(x, np.float32) * F255
        p = np.where(np.isnan(p), np.float32(0), np.clip(p, np.float32(0), F255))
        return p.astype(np.uint8)


def stats(x):
    """(mi, ma) as torch's x.min() / x.max(): a NaN anywhere makes both NaN."""
    x = np.asarray(x, np.float32)
    with np.errstate(invalid="ignore"):
        return np.float32(x.min()), np.float32(x.max())


def normalize(x, mi=None, ma=None):
    """normalize_image in fp32: d = fp32(fp64(ma) - fp64(mi)), or 1e5 when ma == mi;
    (x - mi) / d with an fp32 subtraction and a correctly rounded fp32 division."""
    x = np.asarray(x, np.float32)
    if mi is None:
        mi, ma = stats(x)
    with np.errstate(invalid="ignore"):
        d = np.float32(np.float64(ma) - np.float64(mi)) if ma != mi else np.float32(1e5)
        return ((x - np.float32(mi)) / d).astype(np.float32)


def to_bf16(x):
    """fp32 values rounded to bfloat16 (nearest even), returned widened to fp32 (exact)."""
    u = np.asarray(x, np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32)


def tile_bytes(kind, a):
    """The (h, w, 3) bytes of one tile.  a: colour / warp (3, h, w) fp32; disp / map (h, w)."""
    a = np.asarray(a, np.float32)
    if kind in (COLOR, WARP):
        return quantise(a).transpose(1, 2, 0)
    g = quantise(normalize(a) if kind == DISP else a)
    return np.repeat(g[:, :, None], 3, axis=2)


def build_sheet(n, SH, SW, tiles):
    """tiles: (kind, item, (y, x, h, w), array).  Everything outside the tiles is 0."""
    sheet = np.zeros((n, SH, SW, 3), np.uint8)
    for kind, j, (y, x, h, w), a in tiles:
        b = tile_bytes(kind, a)
        assert b.shape == (h, w, 3), (b.shape, h, w)
        sheet[j, y:y + h, x:x + w] = b
    return sheet


def _np(a):
    """numpy fp32 of an array or of a tensor (any object with .detach().float().cpu().numpy())."""
    return a.detach().float().cpu().numpy() if hasattr(a, "cpu") else np.asarray(a, np.float32)


def expected_sheet(layout, frames, inputs, outputs, warps, n):
    """The sheet of a log step from its tensors.  layout: panel_layout's (SH, SW, tags);
    inputs / outputs: reference-keyed; warps[(source index, 0)]: the fp32 (B, 3, H, W) warped
    colours of scale 0 (md2_generate_images' color_out)."""
    SH, SW, tags = layout
    names = [str(f) for f in frames]
    tiles = []
    for tag, rect in tags.items():
        name, j = tag.rsplit("/", 1)
        j = int(j)
        p = name.split("_")
        s = int(p[-1])
        if name.startswith("color_pred_"):
            tiles.append((WARP, j, rect, _np(warps[(names.index(p[-2]) - 1, 0)][j])))
        elif name.startswith("color_"):
            tiles.append((COLOR, j, rect, _np(inputs[("color", frames[names.index(p[-2])], s)][j])))
        elif name.startswith("disp_"):
            tiles.append((DISP, j, rect, _np(outputs[("disp", s)][j, 0])))
        elif name.startswith("predictive_mask_"):
            tiles.append((MAP, j, rect, _np(outputs["predictive_mask"][("disp", s)][j, names.index(p[-2]) - 1])))
        else:
            tiles.append((MAP, j, rect, _np(outputs["identity_selection/%d" % s][j])))
    return build_sheet(n, SH, SW, tiles)


def quantise_probe():
    """Every k/255, each of them one ulp below and above, and -0.5, 1.5, +-inf, NaN: 773 values."""
    k = (np.arange(256, dtype=np.float64) / 255.0).astype(np.float32)
    below = np.nextafter(k, np.float32(-np.inf)).astype(np.float32)
    above = np.nextafter(k, np.float32(np.inf)).astype(np.float32)
    special = np.array([-0.5, 1.5, np.inf, -np.inf, np.nan], np.float32)
    return np.concatenate([k, below, above, special])


def disp_cases():
    """name -> fp32 (h, w) disparity map (bf16 cases hold bf16-representable values)."""
    rng = np.random.RandomState(31)   # a map on which a multiply by the reciprocal changes a byte
    noise = rng.uniform(0.0, 1.0, (24, 80)).astype(np.float32)
    nan = rng.uniform(0.01, 0.9, (6, 20)).astype(np.float32)
    nan[3, 7] = np.nan
    return {
        "one_1x1": np.array([[0.375]], np.float32),
        "const_5x7": np.full((5, 7), 0.3, np.float32),
        "noise_24x80": noise,
        "tail_4x10": rng.uniform(0.02, 0.7, (4, 10)).astype(np.float32),
        "nan_6x20": nan,
        "bf16_24x80": to_bf16(noise),
    }


def reference_tags(frame_ids, scales, batch, predictive_mask, disable_automasking):
    """The tags of the reference's Trainer.log (trainer.py:547-572), by walking its loops."""
    tags = []
    for j in range(min(4, batch)):
        for s in scales:
            for frame_id in frame_ids:
                tags.append("color_{}_{}/{}".format(frame_id, s, j))
                if s == 0 and frame_id != 0:
                    tags.append("color_pred_{}_{}/{}".format(frame_id, s, j))
            tags.append("disp_{}/{}".format(s, j))
            if predictive_mask:
                for f_idx, frame_id in enumerate(frame_ids[1:]):
                    tags.append("predictive_mask_{}_{}/{}".format(frame_id, s, j))
            elif not disable_automasking:
                tags.append("automask_{}/{}".format(s, j))
    return tags
