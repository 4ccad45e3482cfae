"""The training log's pictures on the device (csrc/md2hot.hip, `md2_log_panel`).

The reference's `Trainer.log` (trainer.py:540-572) hands tensorboard, for the first four
images of the batch, the input frames of every scale, the warped source frames of scale 0,
the min-max normalised disparities (`normalize_image`, utils.py:22-28) and the automask or
the predictive masks.  `log_panel` fills one uint8 contact sheet per image with all of them
in two launches: no warp, sample grid or depth is materialised, nothing returns to the host.
`write_panel` copies the sheet to the host once and writes one PNG per image beside
`scalars.jsonl`.  There is no CPU path: a CPU tensor is an error.

The sheet (`panel_layout`): one band per scale, top to bottom; in a band one
cell per picture, left to right in the order the reference's loops name them — per frame
`color_{f}_{s}` (and behind it `color_pred_{f}_0` in band 0), then `disp_{s}`, then the
`predictive_mask_{f}_{s}` cells or `automask_{s}`.  A cell starts at a multiple of 4 pixels
and the sheet's width is one, so every tile whose own width is a multiple of 4 is written in
whole dwords; a band is as high as its highest cell; the rest of the sheet is 0.
"""
from __future__ import annotations

import ctypes
import json
import os
from typing import Dict, List, Optional, Sequence, Tuple

import torch

from . import _lib
from .hotpath import HotPathConfig

Rect = Tuple[int, int, int, int]   # y, x, h, w


def _up4(v: int) -> int:
    return (v + 3) // 4 * 4


def _cells(cfg: HotPathConfig, frame_ids: Sequence, predictive_mask: bool, automask: bool):
    """Per scale the cells of its band in the reference's order: (name, kind, frame index, (h, w))."""
    bands = []
    for s in range(cfg.num_scales):
        hw = (cfg.height >> s, cfg.width >> s)
        row = []
        for fi, f in enumerate(frame_ids):
            row.append(("color_{}_{}".format(f, s), _lib.LOG_COLOR, fi, hw))
            if s == 0 and fi != 0:
                row.append(("color_pred_{}_{}".format(f, s), _lib.LOG_WARP, fi, hw))
        row.append(("disp_{}".format(s), _lib.LOG_DISP, 0, hw))
        if predictive_mask:
            for fi, f in enumerate(frame_ids[1:]):
                row.append(("predictive_mask_{}_{}".format(f, s), _lib.LOG_MAP, fi + 1, hw))
        elif automask:
            row.append(("automask_{}".format(s), _lib.LOG_MAP, 0, tuple(cfg.loss_res(s))))
        bands.append(row)
    return bands


def _place(cfg, frame_ids, predictive_mask, automask):
    """(SH, SW, [(name, kind, scale, frame index, rect)]) of one item's sheet."""
    out, y, SW = [], 0, 0
    for s, row in enumerate(_cells(cfg, frame_ids, predictive_mask, automask)):
        x = 0
        for name, kind, fi, (h, w) in row:
            out.append((name, kind, s, fi, (y, x, h, w)))
            x += _up4(w)
        SW = max(SW, x)
        y += max(h for _, _, _, (h, _) in row)
    return y, SW, out


def panel_layout(cfg: HotPathConfig, frame_ids: Sequence, items: int = 4, predictive_mask: bool = False,
                 automask: bool = True) -> Tuple[int, int, Dict[str, Rect]]:
    """The single definition of the sheet: (SH, SW, {tag: (y, x, h, w)}) for the first
    min(items, batch) images, a function of the configuration alone.  Tags are the
    reference's (trainer.py:547-572), in the order its loops produce them; the rectangle of
    `name/j` lies in the sheet of image j (every image has the same arrangement)."""
    n = min(int(items), cfg.batch)
    if n < 1:
        raise ValueError("items must be at least 1")
    if len(frame_ids) != 1 + cfg.num_src:
        raise ValueError(f"frame_ids {list(frame_ids)} do not match num_src = {cfg.num_src}")
    SH, SW, placed = _place(cfg, frame_ids, predictive_mask, automask)
    by_scale: Dict[int, list] = {}
    for name, _, s, _, rect in placed:
        by_scale.setdefault(s, []).append((name, rect))
    tags: Dict[str, Rect] = {}
    for j in range(n):
        for s in range(cfg.num_scales):
            for name, rect in by_scale[s]:
                tags["{}/{}".format(name, j)] = rect
    return SH, SW, tags


class PanelPlan:
    """What a log step keeps between calls: the sheet, the workspace and the device copy of
    the tile table.  A call whose tensors sit where the last call's did (a replayed hipGraph's
    static tensors) uploads nothing and allocates nothing."""

    def __init__(self, desc, host: bytes, total_blocks: int, device: torch.device):
        L = _lib.lib()
        self.desc = desc
        self.host = host
        self.total_blocks = total_blocks
        self.table = torch.frombuffer(bytearray(host), dtype=torch.uint8).to(device)
        nbytes = L.md2_log_panel_workspace_bytes(ctypes.byref(desc))
        if nbytes == 0:
            _lib.check(-1, "md2_log_panel_workspace_bytes")
        self.workspace = torch.empty(nbytes, dtype=torch.uint8, device=device)
        self.sheet = torch.empty((desc.items, desc.sheet_h, desc.sheet_w, 3), dtype=torch.uint8, device=device)

    def matches(self, desc, host: bytes, device) -> bool:
        return (bytes(self.desc) == bytes(desc) and self.host == host and self.sheet.device == device)


class LogPanel:
    """One filled sheet.  sheet: uint8 (n, SH, SW, 3) on the device; stats: float32
    (n, num_scales, 2), the minimum and maximum of every logged disparity map; layout:
    panel_layout's triple; images(): tag -> the (h, w, 3) view of the sheet."""

    def __init__(self, plan: PanelPlan, layout, num_scales: int):
        self.plan = plan
        self.sheet = plan.sheet
        self.layout = layout
        n = plan.desc.items
        self.stats = plan.workspace[:n * num_scales * 8].view(torch.float32).view(n, num_scales, 2)

    def images(self) -> Dict[str, torch.Tensor]:
        out = {}
        for tag, (y, x, h, w) in self.layout[2].items():
            j = int(tag.rsplit("/", 1)[1])
            out[tag] = self.sheet[j, y:y + h, x:x + w]
        return out


def _item(t: torch.Tensor, j: int, name: str, shape, device, dtypes=(torch.float32,)) -> torch.Tensor:
    if not torch.is_tensor(t) or not t.is_cuda:
        raise RuntimeError(f"log_panel is GPU only (HIP kernels, no CPU fallback): {name} is not a device tensor")
    if t.device != device or t.dtype not in dtypes or tuple(t.shape[1:]) != tuple(shape):
        raise ValueError(f"{name} must be {dtypes} (B, {', '.join(map(str, shape))}) on {device}, got {t.dtype} "
                         f"{tuple(t.shape)} on {t.device}")
    return t.detach().contiguous()[j]


def run_tiles(cfg: HotPathConfig, n: int, sheet_hw: Sequence[int], layout_tags: Dict[str, Rect],
              specs: List[tuple], disps: Sequence[torch.Tensor], warp: Optional[dict] = None,
              plan: Optional[PanelPlan] = None) -> LogPanel:
    """The operator under a table the caller states: specs are (kind, item, scale, frame
    index, (y, x, h, w), source tensor) and disps the per-scale disparity batches (the
    statistics' source).  warp: {"colors0": [target, sources...], "K": K[0], "inv_K":
    inv_K[0], "T": T} when the table holds warp tiles.  log_panel builds its table from
    panel_layout and calls this."""
    L = _lib.lib()
    dev = disps[0].device
    if dev.type != "cuda":
        raise RuntimeError("log_panel is GPU only (HIP kernels, no CPU fallback); got device " + str(dev))
    disps = [d.detach().contiguous() for d in disps]
    st = _lib.Tensors()
    keep = list(disps)
    for s, d in enumerate(disps):
        st.disp[s] = d.data_ptr()
    if warp is not None:
        cols = [c.detach().contiguous() for c in warp["colors0"]]
        K, iK, T = (warp[k].detach().contiguous() for k in ("K", "inv_K", "T"))
        keep += cols + [K, iK, T]
        for fi, c in enumerate(cols):
            st.color[0][fi] = c.data_ptr()
        st.K[0], st.inv_K[0], st.T = K.data_ptr(), iK.data_ptr(), T.data_ptr()
    table = (_lib.LogTile * len(specs))()
    blocks = 0
    for i, (kind, j, s, fi, (y, x, h, w), src) in enumerate(specs):
        keep.append(src)
        table[i] = _lib.LogTile(kind, j, s, fi, y, x, h, w, src.data_ptr(), blocks, 0)
        blocks += L.md2_log_panel_tile_blocks(ctypes.byref(table[i]))
    desc = _lib.LogDesc(cfg.desc(0, disps[0].dtype), n, int(sheet_hw[0]), int(sheet_hw[1]), len(specs))
    host = bytes(table)
    if plan is None or not plan.matches(desc, host, dev):
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("log_panel under capture needs the plan of an eager call on the same tensors")
        _lib.check(L.md2_log_panel_check(ctypes.byref(desc), table, ctypes.byref(st)), "md2_log_panel_check")
        plan = PanelPlan(desc, host, blocks, dev)
    _lib.check(L.md2_log_panel(ctypes.byref(desc), ctypes.byref(st), plan.table.data_ptr(), plan.total_blocks,
                               plan.sheet.data_ptr(), plan.workspace.data_ptr(), _lib.stream(dev)), "md2_log_panel")
    del keep   # temporaries made contiguous above: the allocator reuses them in stream order, behind the launches
    return LogPanel(plan, (int(sheet_hw[0]), int(sheet_hw[1]), layout_tags), cfg.num_scales)


def log_panel(cfg: HotPathConfig, inputs: Dict, outputs: Dict, frame_ids: Sequence, T: torch.Tensor,
              items: int = 4, plan: Optional[PanelPlan] = None) -> LogPanel:
    """The contact sheet of one step from what the step holds: `inputs` (the colour
    pyramids, K, inv_K), `outputs` (disparities, the predictive masks or the
    identity_selection maps of compute_losses) and the stacked cam_T_cam `T` the hot path
    took ((S,B,4,4), or (num_scales,S,B,4,4) with cfg.t_per_scale: the scale-0 transforms are
    used, as generate_images_pred does).  No host synchronisation; pass the returned
    panel's `.plan` to the next call to reuse its buffers (required under hipGraph capture)."""
    dev = T.device
    if dev.type != "cuda":
        raise RuntimeError("log_panel is GPU only (HIP kernels, no CPU fallback); got device " + str(dev))
    n = min(int(items), cfg.batch)
    automask = not cfg.disable_automasking
    SH, SW, tags = panel_layout(cfg, frame_ids, n, cfg.predictive_mask, automask)
    _, _, placed = _place(cfg, frame_ids, cfg.predictive_mask, automask)
    H, W = cfg.height, cfg.width
    ddt = (torch.float32, torch.bfloat16)
    disps = [outputs[("disp", s)] for s in range(cfg.num_scales)]
    specs = []
    for j in range(n):
        for name, kind, s, fi, rect in placed:
            hw = (H >> s, W >> s)
            if kind == _lib.LOG_COLOR:
                src = _item(inputs[("color", frame_ids[fi], s)], j, name, (3,) + hw, dev)
            elif kind == _lib.LOG_WARP:
                src = _item(inputs[("color", frame_ids[fi], 0)], j, name, (3, H, W), dev)
            elif kind == _lib.LOG_DISP:
                src = _item(disps[s], j, name, (1,) + hw, dev, ddt)
            elif cfg.predictive_mask:
                src = _item(outputs["predictive_mask"][("disp", s)], j, name, (cfg.num_src,) + hw, dev)[fi - 1]
            else:
                src = _item(outputs["identity_selection/{}".format(s)], j, name, cfg.loss_res(s), dev)
            specs.append((kind, j, s, fi, rect, src))
    tshape = (cfg.num_scales, cfg.num_src, cfg.batch, 4, 4) if cfg.t_per_scale else (cfg.num_src, cfg.batch, 4, 4)
    if tuple(T.shape) != tshape or T.dtype != torch.float32:
        raise ValueError(f"T must be float32 {tshape}, got {T.dtype} {tuple(T.shape)}")
    warp = {"colors0": [inputs[("color", f, 0)] for f in frame_ids], "K": inputs[("K", 0)],
            "inv_K": inputs[("inv_K", 0)], "T": T}
    return run_tiles(cfg, n, (SH, SW), tags, specs, disps, warp, plan)


def write_panel(panel: LogPanel, folder: str, step: int, device_encode: bool = False) -> List[str]:
    """step_{step:07d}_{j}.png per logged image under `folder`, and once per folder
    layout.json (tag -> [y, x, h, w]).  The one copy of the sheet to the host is the only
    synchronisation of a log step's pictures.  device_encode: the sheet is filtered and
    deflated on the device (png_ops.encode_png_batch) and the compressed bytes
    are what is copied: the same pixels in files of other bytes."""
    os.makedirs(folder, exist_ok=True)
    paths = []
    if device_encode:
        from . import png_ops
        for j, data in enumerate(png_ops.encode_png_batch(panel.sheet, kind=png_ops.KIND_RGB8)):
            p = os.path.join(folder, "step_{:07d}_{}.png".format(int(step), j))
            with open(p, "wb") as f:
                f.write(data)
            paths.append(p)
    else:
        from PIL import Image
        host = panel.sheet.cpu().numpy()
        for j in range(host.shape[0]):
            p = os.path.join(folder, "step_{:07d}_{}.png".format(int(step), j))
            Image.fromarray(host[j]).save(p)
            paths.append(p)
    lj = os.path.join(folder, "layout.json")
    if not os.path.exists(lj):
        with open(lj, "w") as f:
            json.dump({tag: list(rect) for tag, rect in panel.layout[2].items()}, f, indent=1)
    return paths
