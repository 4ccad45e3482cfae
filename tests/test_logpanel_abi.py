"""CPU-side checks of the training log's contact sheet (md2_log_panel, csrc/md2hot.hip):
the symbols and struct layouts, every refusal of the host-only validator (no kernel is
launched), panel_layout over the ablation matrix, and the numpy restatement
(tests/logpanel_case.py) against the recorded results of the reference's normalize_image."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch  # noqa: F401  (load order: torch's HIP runtime first)

from monodepth2_amd import _lib
from monodepth2_amd.build import build
from monodepth2_amd.hotpath import HotPathConfig
from monodepth2_amd.log_ops import log_panel, panel_layout

import logpanel_case as lc

HERE = os.path.dirname(os.path.abspath(__file__))
HEADER = os.path.join(os.path.dirname(HERE), "include", "md2hot.h")
SYMBOLS = ["md2_log_panel_tile_blocks", "md2_log_panel_check", "md2_log_panel_workspace_bytes", "md2_log_panel"]


@pytest.fixture(scope="module")
def L():
    build()
    return _lib.lib()


def test_symbols_structs_and_abi(L):
    text = open(HEADER).read()
    for sym in SYMBOLS:
        assert re.search(r"\b%s\(" % sym, text), sym
        assert sym in _lib.EXPORTS and hasattr(L, sym)
    for name in ("md2_log_tile", "md2_log_desc", "MD2_LOG_COLOR", "MD2_LOG_WARP", "MD2_LOG_DISP", "MD2_LOG_MAP"):
        assert name in text
    assert "#define MD2_ABI_VERSION 24" in text
    assert L.md2_abi_version() == 24 == _lib.ABI_VERSION   # new symbols only: no bump
    T, D = _lib.LogTile, _lib.LogDesc
    assert ctypes.sizeof(T) == 48 and ctypes.sizeof(D) == 64 and ctypes.sizeof(_lib.Desc) == 48
    assert [getattr(T, f).offset for f in ("kind", "item", "scale", "frame", "y", "x", "h", "w", "src", "block0",
                                           "reserved")] == [0, 4, 8, 12, 16, 20, 24, 28, 32, 40, 44]
    assert [getattr(D, f).offset for f in ("hot", "items", "sheet_h", "sheet_w", "num_tiles")] == [0, 48, 52, 56, 60]
    assert (_lib.LOG_COLOR, _lib.LOG_WARP, _lib.LOG_DISP, _lib.LOG_MAP) == (0, 1, 2, 3)
    # the header states the sizes the binding relies on
    assert "the struct is 48 bytes" in text and "the struct is 64 bytes" in text


def cfg_of(name, B=2, H=64, W=128):
    frames = {"mono": [0, -1, 1], "stereo": [0, -1, 1, "s"], "stereo_only": [0, "s"]}.get(name, [0, -1, 1])
    kw = dict(posecnn=dict(t_per_scale=True), v1_multiscale=dict(v1_multiscale=True),
              predictive_mask=dict(predictive_mask=True, disable_automasking=True),
              disable_automasking=dict(disable_automasking=True)).get(name, {})
    return HotPathConfig(batch=B, height=H, width=W, num_src=len(frames) - 1, **kw), frames


ABLATIONS = ["mono", "stereo", "stereo_only", "posecnn", "v1_multiscale", "predictive_mask", "disable_automasking"]


def table_of(L, cfg, frames, items=4):
    """panel_layout's own table with a dummy (never dereferenced) source per tile."""
    n = min(items, cfg.batch)
    SH, SW, tags = panel_layout(cfg, frames, items, cfg.predictive_mask, not cfg.disable_automasking)
    tiles = (_lib.LogTile * len(tags))()
    blocks = 0
    for i, (tag, (y, x, h, w)) in enumerate(tags.items()):
        name, j = tag.rsplit("/", 1)
        kind = (_lib.LOG_WARP if name.startswith("color_pred_") else _lib.LOG_COLOR if name.startswith("color_")
                else _lib.LOG_DISP if name.startswith("disp_") else _lib.LOG_MAP)
        parts = name.split("_")
        s = int(parts[-1])
        f = 0
        if kind in (_lib.LOG_COLOR, _lib.LOG_WARP) or name.startswith("predictive_mask_"):
            f = [str(v) for v in frames].index(parts[-2])
        tiles[i] = _lib.LogTile(kind, int(j), s, f, y, x, h, w, 256, blocks, 0)
        blocks += L.md2_log_panel_tile_blocks(ctypes.byref(tiles[i]))
    desc = _lib.LogDesc(cfg.desc(), n, SH, SW, len(tags))
    return desc, tiles, blocks


def tensors(S=2):
    st = _lib.Tensors()
    st.T = st.disp[0] = st.K[0] = st.inv_K[0] = 256
    for f in range(1, S + 1):
        st.color[0][f] = 256
    return st


@pytest.mark.parametrize("B", [1, 3, 5])
@pytest.mark.parametrize("name", ABLATIONS)
def test_the_layouts_own_tables_pass_the_validator(L, name, B):
    cfg, frames = cfg_of(name, B)
    desc, tiles, blocks = table_of(L, cfg, frames)
    st = tensors(cfg.num_src)
    assert L.md2_log_panel_check(ctypes.byref(desc), tiles, ctypes.byref(st)) == 0, L.md2_last_error().decode()
    assert desc.items == min(4, B) and blocks > 0
    assert L.md2_log_panel_workspace_bytes(ctypes.byref(desc)) == 256


@pytest.mark.parametrize("B", [1, 3, 5])
@pytest.mark.parametrize("name", ABLATIONS)
def test_layout_tags_are_the_references_and_rectangles_are_disjoint(name, B):
    cfg, frames = cfg_of(name, B)
    SH, SW, tags = panel_layout(cfg, frames, 4, cfg.predictive_mask, not cfg.disable_automasking)
    assert list(tags) == lc.reference_tags(frames, range(4), B, cfg.predictive_mask, cfg.disable_automasking)
    assert panel_layout(cfg, frames, 4, cfg.predictive_mask, not cfg.disable_automasking) == (SH, SW, tags)
    assert SW % 4 == 0
    for j in range(min(4, B)):
        cover = np.zeros((SH, SW), np.int32)
        for tag, (y, x, h, w) in tags.items():
            if tag.endswith("/%d" % j):
                assert 0 <= y and 0 <= x and y + h <= SH and x + w <= SW and x % 4 == 0, tag
                cover[y:y + h, x:x + w] += 1
        assert cover.max() == 1
    sizes = {t.rsplit("/", 1)[0]: r[2:] for t, r in tags.items()}
    for s in range(4):
        assert sizes["disp_%d" % s] == sizes["color_0_%d" % s] == (cfg.height >> s, cfg.width >> s)
        if not cfg.disable_automasking:
            assert sizes["automask_%d" % s] == tuple(cfg.loss_res(s))
    assert sizes["color_pred_%s_0" % frames[1]] == (cfg.height, cfg.width)


def refused(L, desc, tiles, st, msg):
    assert L.md2_log_panel_check(ctypes.byref(desc), tiles, ctypes.byref(st) if st is not None else None) == -1
    err = L.md2_last_error().decode()
    assert msg in err and "log_panel" in err, err


def test_every_refusal_of_the_validator(L):
    cfg, frames = cfg_of("mono", 5)
    st = tensors()
    first = {}
    desc, tiles, _ = table_of(L, cfg, frames)
    for i, t in enumerate(tiles):
        first.setdefault(t.kind, i)

    def fresh():
        return table_of(L, cfg, frames)[:2]

    for items in (0, 5, -1):
        d, t = fresh()
        d.items = items
        refused(L, d, t, st, "items must be")
    d, t = table_of(L, cfg_of("mono", 3)[0], frames)[:2]
    d.items = 4                                          # above batch = 3
    refused(L, d, t, st, "items must be")
    d, t = fresh()
    d.sheet_w = t[first[_lib.LOG_COLOR]].w - 1           # the first tile leaves the sheet
    refused(L, d, t, st, "leaves the")
    d, t = fresh()
    t[3].y += d.sheet_h
    refused(L, d, t, st, "leaves the")
    d, t = fresh()
    t[1].x = t[0].x + 4                                  # into its neighbour
    refused(L, d, t, st, "overlap")
    for kind in (_lib.LOG_COLOR, _lib.LOG_WARP, _lib.LOG_DISP, _lib.LOG_MAP):
        d, t = fresh()
        t[first[kind]].h -= 1
        refused(L, d, t, st, "needs")
    d, t = fresh()
    i = next(k for k, e in enumerate(t) if e.kind == _lib.LOG_DISP and e.scale == 1)
    t[i].scale = 2                                       # a scale-1 sized tile named scale 2
    refused(L, d, t, st, "needs")
    d, t = fresh()
    t[first[_lib.LOG_WARP]].scale = 1
    refused(L, d, t, st, "scale 0 only")
    for frame in (-1, 3):
        d, t = fresh()
        t[first[_lib.LOG_COLOR]].frame = frame
        refused(L, d, t, st, "frame index")
    d, t = fresh()
    t[first[_lib.LOG_WARP]].frame = 0                    # the target is not warped
    refused(L, d, t, st, "frame index")
    d, t = fresh()
    t[5].src = None
    refused(L, d, t, st, "NULL src")
    d, t = fresh()
    t[2].kind = 4
    refused(L, d, t, st, "unknown kind")
    d, t = fresh()
    t[2].item = 4
    refused(L, d, t, st, "names item")
    d, t = fresh()
    t[2].block0 += 1
    refused(L, d, t, st, "running sum")
    d, t = fresh()
    refused(L, d, t, None, "needs tensors")
    bad = tensors()
    bad.T = None
    refused(L, d, t, bad, "needs T")
    bad = tensors()
    bad.color[0][2] = None
    refused(L, d, t, bad, "color[0][2]")
    assert L.md2_log_panel_check(None, t, ctypes.byref(st)) == -1 and "NULL desc" in L.md2_last_error().decode()
    assert L.md2_log_panel_check(ctypes.byref(d), None, ctypes.byref(st)) == -1
    assert "NULL tile table" in L.md2_last_error().decode()
    d, t = fresh()
    d.num_tiles = 0
    refused(L, d, t, st, "num_tiles")
    assert L.md2_log_panel_workspace_bytes(ctypes.byref(d)) == 0
    # md2_log_panel refuses the same descriptors, a NULL operand and misaligned buffers before any launch
    x = ctypes.c_void_p(256)
    assert L.md2_log_panel(ctypes.byref(d), ctypes.byref(st), x, 1, x, x, None) == -1
    d, t = fresh()
    assert L.md2_log_panel(ctypes.byref(d), ctypes.byref(st), None, 1, x, x, None) == -1
    assert "NULL operand" in L.md2_last_error().decode()
    assert L.md2_log_panel(ctypes.byref(d), ctypes.byref(st), x, 1, ctypes.c_void_p(264), x, None) == -1
    assert "aligned" in L.md2_last_error().decode()
    assert L.md2_log_panel(ctypes.byref(d), ctypes.byref(st), x, 0, x, x, None) == -1
    assert "total_blocks" in L.md2_last_error().decode()


def test_a_table_without_warps_needs_no_tensors_and_any_positive_size(L):
    cfg = HotPathConfig(batch=1, height=1, width=1, num_src=1, num_scales=1)
    t = (_lib.LogTile * 1)(_lib.LogTile(_lib.LOG_DISP, 0, 0, 0, 0, 0, 1, 1, 256, 0, 0))
    d = _lib.LogDesc(cfg.desc(), 1, 1, 4, 1)
    assert L.md2_log_panel_check(ctypes.byref(d), t, None) == 0, L.md2_last_error().decode()
    assert L.md2_log_panel_tile_blocks(ctypes.byref(t[0])) == 1
    big = _lib.LogTile(_lib.LOG_COLOR, 0, 0, 0, 0, 0, 192, 642, 256, 0, 0)
    assert L.md2_log_panel_tile_blocks(ctypes.byref(big)) == (192 * 161 + 255) // 256
    t[0].kind = _lib.LOG_WARP
    t[0].frame = 1
    refused(L, d, t, tensors(1), "smaller than 2 x 2")


def test_there_is_no_cpu_path():
    cfg, frames = cfg_of("mono")
    with pytest.raises(RuntimeError, match="GPU only"):
        log_panel(cfg, {}, {}, frames, torch.zeros(2, 2, 4, 4))


def test_the_restatement_against_the_recorded_reference():
    z = np.load(os.path.join(HERE, "golden", "logpanel", "logpanel.npz"))
    cases = lc.disp_cases()
    assert list(z["names"]) == list(cases)
    for name, x in cases.items():
        assert np.array_equal(z["in_" + name], x, equal_nan=True), name
        got = lc.normalize(x)
        assert np.array_equal(got.view(np.uint32), z["norm_" + name].view(np.uint32)) or np.isnan(x).any(), name
        assert np.array_equal(np.isnan(got), np.isnan(z["norm_" + name]))
        assert np.array_equal(np.array(lc.stats(x)), z["stats_" + name], equal_nan=True), name
        assert np.array_equal(lc.tile_bytes(lc.DISP, x)[:, :, 0], z["bytes_" + name]), name
    assert (z["bytes_const_5x7"] == 0).all() and (z["bytes_nan_6x20"] == 0).all() and z["bytes_one_1x1"][0, 0] == 0
    assert z["bytes_noise_24x80"].max() == 255 and z["bytes_noise_24x80"].min() == 0
    # the case a multiply by the reciprocal fails: it moves a byte of the 24 x 80 map
    x = cases["noise_24x80"]
    mi, ma = lc.stats(x)
    recip = (x - mi) * (np.float32(1) / np.float32(np.float64(ma) - np.float64(mi)))
    assert (lc.quantise(recip) != z["bytes_noise_24x80"]).sum() >= 1


def test_quantise_round_trips_every_byte():
    probe = lc.quantise_probe()
    q = lc.quantise(probe)
    assert np.array_equal(q[:256], np.arange(256))
    assert np.array_equal(q[512:768], np.arange(256))                 # one ulp above: the same byte
    assert np.array_equal(q[257:512], np.arange(255))                 # one ulp below: the byte before
    assert q[256] == 0 and list(q[768:]) == [0, 255, 255, 0, 0]
