"""CPU-side checks of the point-cloud ABI (md2_depth_points, csrc/points.hip): struct
layout, every refusal and its message through both entry points, workspace sizes — no
kernel is launched — `write_ply`, the command's argument parsing, pose count check and pose
chain, and the pin of the tests' numpy restatement (tests/points_case.py) to the golden
captured from the reference's disp_to_depth and BackprojectDepth
(tests/golden/points/make_points_golden.py)."""
import ctypes
import functools

import numpy as np
import pytest
import torch  # noqa: F401  (load order: torch's HIP runtime first)

from monodepth2_amd import _lib
from monodepth2_amd import points_ops as po
from monodepth2_amd.build import SOURCES, build

import points_case as pc


@pytest.fixture(scope="module")
def L():
    build()
    return _lib.lib()


@pytest.fixture(scope="module")
def golden():
    return pc.load_golden()


def test_struct_layout_and_abi(L):
    D = _lib.PointsDesc
    assert ctypes.sizeof(D) == 48
    assert (D.batch.offset, D.height.offset, D.width.offset, D.stride.offset) == (0, 4, 8, 12)
    assert (D.disp_a.offset, D.disp_b.offset, D.depth_scale.offset) == (16, 20, 24)
    assert (D.near.offset, D.far.offset, D.flags.offset, D.reserved.offset) == (28, 32, 36, 40)
    assert (_lib.POINTS_DEPTH_INPUT, _lib.POINTS_WORLD, po.RECORD_BYTES) == (1, 2, 15)
    assert L.md2_abi_version() == 24 == _lib.ABI_VERSION   # new symbols only: no bump
    assert {"md2_depth_points", "md2_depth_points_workspace_bytes"} <= set(_lib.EXPORTS)
    assert hasattr(L, "md2_depth_points") and hasattr(L, "md2_depth_points_workspace_bytes")
    assert "points.hip" in SOURCES
    assert po.VERTEX_DTYPE == pc.VERTEX and po.VERTEX_DTYPE.itemsize == 15


def desc(**kw):
    args = dict(batch=3, height=37, width=50)
    args.update(kw)
    return po.points_desc(**args)


X = ctypes.c_void_p(256)          # non-NULL, 256-byte aligned, never dereferenced


def call(L, d, map=X, rgb=X, inv_K=X, T=None, vertices=X, capacity=None, offsets=X, workspace=X):
    if capacity is None:
        capacity = po.capacity(d.batch, d.height, d.width, d.stride) if d is not None and d.stride > 0 else 0
    return L.md2_depth_points(ctypes.byref(d) if d is not None else None, map, rgb, inv_K, T, vertices, capacity,
                              offsets, workspace, None)


INF, NAN = float("inf"), float("nan")
BAD = [
    (dict(batch=0), "must be positive"),
    (dict(batch=-1), "must be positive"),
    (dict(height=0), "must be positive"),
    (dict(width=-5), "must be positive"),
    (dict(stride=0), "must be positive"),
    (dict(stride=-2), "must be positive"),
    (dict(batch=65536), "65535"),                                   # images are grid.y
    (dict(batch=1, height=2 ** 16, width=2 ** 15), "2^31"),
    (dict(batch=2, height=2 ** 15, width=2 ** 15), "2^31"),
    (dict(batch=65535, height=2 ** 31 - 1, width=2 ** 31 - 1), "2^31"),   # past int64 if multiplied naively
    (dict(batch=1, height=2 ** 31 - 1, width=2 ** 31 - 1, stride=46340), "2^31"),   # 46342^2 > 2^31
    (dict(near=0.0), "near"),
    (dict(near=-1.0), "near"),
    (dict(near=NAN), "near"),
    (dict(far=INF), "far"),
    (dict(far=NAN), "far"),
    (dict(near=INF), "near"),
    (dict(near=2.0, far=1.0), "near"),
    (dict(depth_scale=0.0), "depth_scale"),
    (dict(depth_scale=-5.4), "depth_scale"),
    (dict(depth_scale=INF), "depth_scale"),
    (dict(depth_scale=NAN), "depth_scale"),
]


@pytest.mark.parametrize("kw,msg", BAD)
def test_invalid_desc_is_refused_with_a_message(L, kw, msg):
    d = desc(**kw)
    assert L.md2_depth_points_workspace_bytes(ctypes.byref(d)) == 0
    assert msg in L.md2_last_error().decode()
    assert call(L, d, capacity=2 ** 40) == -1
    assert msg in L.md2_last_error().decode()
    with pytest.raises(RuntimeError, match="md2_depth_points_workspace_bytes"):
        po.workspace_bytes(d.batch, d.height, d.width, near=d.near, far=d.far, depth_scale=d.depth_scale,
                           stride=d.stride)


def test_flags_and_reserved_words(L):
    for bit in (4, 8, 1 << 31):
        d = desc()
        d.flags = bit
        assert L.md2_depth_points_workspace_bytes(ctypes.byref(d)) == 0
        assert "unknown flags" in L.md2_last_error().decode()
        assert call(L, d) == -1
        assert "unknown flags" in L.md2_last_error().decode()
    for word in (0, 1):
        d = desc()
        d.reserved[word] = 1
        assert L.md2_depth_points_workspace_bytes(ctypes.byref(d)) == 0
        assert "reserved" in L.md2_last_error().decode()
        assert call(L, d) == -1
        assert "reserved" in L.md2_last_error().decode()
    for kw in (dict(depth_input=True), dict(world=True), dict(depth_input=True, world=True)):
        assert L.md2_depth_points_workspace_bytes(ctypes.byref(desc(**kw))) > 0


def test_null_desc_and_operands(L):
    assert L.md2_depth_points_workspace_bytes(None) == 0
    assert "NULL desc" in L.md2_last_error().decode()
    assert call(L, None) == -1
    assert "NULL desc" in L.md2_last_error().decode()
    d = desc()
    for hole in ("map", "rgb", "inv_K", "vertices", "offsets", "workspace"):
        assert call(L, d, **{hole: None}) == -1
        assert "NULL operand" in L.md2_last_error().decode()


def test_T_must_agree_with_the_flag(L):
    assert call(L, desc(world=True), T=None) == -1
    assert "needs T" in L.md2_last_error().decode()
    assert call(L, desc(), T=X) == -1
    assert "T must be NULL" in L.md2_last_error().decode()


def test_capacity_and_workspace_alignment(L):
    d = desc(stride=3)                       # 3 * 13 * 17 candidates
    need = 3 * 13 * 17
    assert po.capacity(3, 37, 50, 3) == need
    for cap in (0, 1, need - 1):
        assert call(L, d, capacity=cap) == -1
        assert "capacity" in L.md2_last_error().decode()
    for off in (8, 16, 128):
        assert call(L, desc(), workspace=ctypes.c_void_p(256 + off)) == -1
        assert "256-byte aligned" in L.md2_last_error().decode()


def test_the_largest_legal_sizes_are_accepted(L):
    ws = L.md2_depth_points_workspace_bytes
    assert ws(ctypes.byref(desc(batch=65535, height=128, width=255))) > 0            # 65535 * 32640 < 2^31
    assert ws(ctypes.byref(desc(batch=1, height=46340, width=46340))) > 0            # 46340^2 < 2^31
    assert ws(ctypes.byref(desc(batch=1, height=1, width=2 ** 31 - 1))) > 0
    assert ws(ctypes.byref(desc(batch=65535, height=2 ** 31 - 1, width=2 ** 31 - 1, stride=2 ** 31 - 1))) > 0
    assert ws(ctypes.byref(desc(batch=1, height=1, width=1, near=1e-30, far=3e38, depth_scale=3e38))) > 0
    assert ws(ctypes.byref(desc(near=5.0, far=5.0))) > 0                             # near == far is a range


def test_workspace_is_monotone_in_batch_and_size(L):
    def ws(batch, hw, stride=1):
        n = L.md2_depth_points_workspace_bytes(ctypes.byref(desc(batch=batch, height=hw[0], width=hw[1],
                                                                  stride=stride)))
        assert n > 0 and n % 256 == 0
        return n

    by_batch = [ws(b, (37, 50)) for b in (1, 64, 65, 697, 65535)]
    assert all(a <= b for a, b in zip(by_batch, by_batch[1:])) and by_batch[0] < by_batch[2] < by_batch[-1], by_batch
    by_size = [ws(16, s) for s in ((1, 1), (3, 5), (37, 50), (192, 640), (375, 1242), (4096, 4096))]
    assert all(a <= b for a, b in zip(by_size, by_size[1:])) and by_size[0] < by_size[3] < by_size[-1], by_size
    assert ws(16, (375, 1242), 2) <= ws(16, (375, 1242)) and ws(16, (375, 1242), 4) < ws(16, (375, 1242))
    # neither the scalars nor the flags enter
    assert po.workspace_bytes(3, 37, 50) == po.workspace_bytes(3, 37, 50, depth_input=True, world=True, far=9.0)


def test_depth_to_points_has_no_cpu_fallback_and_checks_its_input():
    m, rgb, k = torch.zeros(1, 4, 4), torch.zeros(1, 4, 4, 3, dtype=torch.uint8), torch.eye(4)[None]
    with pytest.raises(RuntimeError, match="GPU only"):
        po.depth_to_points(m, rgb, k)
    with pytest.raises(RuntimeError, match="GPU only"):
        po.depth_to_points(np.zeros((1, 4, 4), np.float32), rgb, k)


def test_disp_scalars_are_rounded_once_from_double():
    d = desc(min_depth=0.1, max_depth=100.0)
    a, b = pc.disp_scalars()
    assert np.float32(d.disp_a) == a == np.float32(9.99) and np.float32(d.disp_b) == b == np.float32(0.01)
    d = desc(depth_input=True)
    assert (d.disp_a, d.disp_b, d.flags) == (0.0, 0.0, 1)


def test_write_ply_header_and_body(tmp_path):
    rec = np.zeros(5, pc.VERTEX)
    rec["x"], rec["y"], rec["z"] = np.arange(5) + 0.5, -np.arange(5), 1e-3
    rec["red"], rec["green"], rec["blue"] = 255, np.arange(5), 7
    body = np.concatenate([rec.view(np.uint8), np.full(30, 0xA5, np.uint8)])     # a longer buffer: only 5 go out
    path = tmp_path / "five.ply"
    po.write_ply(path, body, 5)
    data = path.read_bytes()
    header = (b"ply\nformat binary_little_endian 1.0\nelement vertex 5\nproperty float x\nproperty float y\n"
              b"property float z\nproperty uchar red\nproperty uchar green\nproperty uchar blue\nend_header\n")
    assert data.startswith(header) and len(data) == len(header) + 75
    assert np.array_equal(np.frombuffer(data[len(header):], pc.VERTEX), rec)
    assert np.array_equal(po.read_ply(path), rec)
    po.write_ply(path, torch.from_numpy(body), 0)                                  # an empty cloud is a file too
    assert path.read_bytes() == header.replace(b"vertex 5", b"vertex 0") and po.read_ply(path).size == 0
    po.write_ply(path, rec.tobytes(), 2)
    assert np.array_equal(po.read_ply(path), rec[:2])
    with pytest.raises(ValueError, match="need 90 bytes"):
        po.write_ply(path, rec.view(np.uint8), 6)
    with pytest.raises(ValueError, match="uint8"):
        po.write_ply(path, np.zeros(30, np.float32), 1)


def test_command_arguments_pose_count_and_pose_chain():
    from monodepth2_amd import pointcloud as cmd
    args = cmd.parse_args(["--image_path", "x", "--load_weights_folder", "w"])
    assert (args.ext, args.num_layers, args.pred_metric_depth, args.stride) == ("jpg", 18, False, 1)
    assert (args.near, args.far, args.poses, args.out) == (1e-3, 80.0, None, None)
    assert args.intrinsics == [np.float32(0.58), np.float32(1.92), 0.5, 0.5]      # KITTIDataset.K's fp32 values
    args = cmd.parse_args(["--image_path", "x", "--load_weights_folder", "w", "--intrinsics", "0.6", "1.9", "0.4",
                           "0.45", "--stride", "3", "--near", "0.5", "--far", "30", "--poses", "p.npy", "--out",
                           "c.ply", "--pred_metric_depth"])
    assert (args.intrinsics, args.stride, args.near, args.far) == ([0.6, 1.9, 0.4, 0.45], 3, 0.5, 30.0)
    assert (args.poses, args.out, args.pred_metric_depth) == ("p.npy", "c.ply", True)
    for bad in (["--poses", "p.npy"], ["--out", "c.ply"], ["--stride", "0"], ["--model_name", "mono_640x192"],
                ["--intrinsics", "1", "2", "3"]):
        with pytest.raises(SystemExit):
            cmd.parse_args(["--image_path", "x", "--load_weights_folder", "w"] + bad)

    cmd.check_pose_count(2, 3)
    with pytest.raises(SystemExit, match="holds 4 transforms but 3 images"):
        cmd.check_pose_count(4, 3)
    with pytest.raises(SystemExit, match="holds 2 transforms but 2 images"):
        cmd.check_pose_count(2, 2)
    with pytest.raises(SystemExit, match=r"\(N-1,4,4\)"):
        cmd.chain_poses(np.zeros((3, 3, 4), np.float32))

    # the reference's dump_xyz rule, literally: cam_to_world = I; cam_to_world = cam_to_world . P
    poses = pc.rigid(6, 5, reach=2.0)
    chain = cmd.chain_poses(poses)
    assert chain.shape == (7, 4, 4) and chain.dtype == np.float32
    cam_to_world = np.eye(4)
    assert np.array_equal(chain[0], np.eye(4, dtype=np.float32))
    for i, p in enumerate(poses):
        cam_to_world = np.dot(cam_to_world, p.astype(np.float64))
        assert np.array_equal(chain[i + 1], cam_to_world.astype(np.float32))

    # the intrinsics as mono_dataset.py builds them
    K, inv_K = pc.intrinsics(37, 50)
    mine = cmd.inverse_intrinsics(cmd.DEFAULT_INTRINSICS, 37, 50)
    assert mine.dtype == np.float32 and np.array_equal(mine, inv_K[0])


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def test_golden_is_complete(golden):
    names = [str(n) for n in golden["names"]]
    assert names == list(pc.golden_cases()) == ["g_1x5x7", "g_3x37x50", "g_1x64x128"]
    for name, (disp, inv_K, K) in pc.golden_cases().items():        # the inputs are regenerated identically
        c = pc.case(golden, name)
        assert np.array_equal(bits(c["disp"]), bits(disp)) and np.array_equal(bits(c["inv_K"]), bits(inv_K))
        assert np.array_equal(c["K"], K) and c["cam"].shape == disp.shape[:1] + (3,) + disp.shape[1:]
        assert c["cam"].dtype == np.float32 and c["f64"].dtype == np.float64 and 0 < c["floor"] < 1e-6
    assert golden["sizes"].tolist() == [[192, 640], [375, 1242]] and golden["measured"].shape == (2, 5)


@pytest.mark.parametrize("name", list(pc.golden_cases()))
def test_restatement_against_the_golden(golden, name):
    """The restatement's depth is the reference's bit for bit; its coordinates lie within 4
    floors of the fp64 evaluation (torch's matmul rounds the same sum in another order:
    the repository's convention for such a formula); reprojecting the records with K gives
    the pixel indices back within 0.01 px — 50 times below the half pixel a wrong
    pixel-centre convention costs."""
    c = pc.case(golden, name)
    depth = pc.depth_np(c["disp"])
    assert np.array_equal(bits(depth), bits(c["depth"]))
    z, P = pc.camera_points_np(depth, c["inv_K"])
    assert np.array_equal(bits(z), bits(depth))                                      # depth_scale 1
    scale = np.abs(c["f64"]).max(axis=1)
    err = float((np.abs(P.astype(np.float64) - c["f64"]).max(axis=1) / scale).max())
    same = float((bits(P) == bits(c["cam"])).mean())
    B, H, W = c["disp"].shape
    rec, offsets, keep, _ = pc.points_np(c["disp"], pc.colours(B, H, W, 0), c["inv_K"], far=np.inf)
    assert keep.all() and offsets.tolist() == [H * W * b for b in range(B + 1)]
    u, v = pc.reproject_np(rec, c["K"][0])
    _, y, x = np.nonzero(keep)
    px = float(max(np.abs(u - x).max(), np.abs(v - y).max()))
    print(name, "restatement vs fp64", err, "floor", c["floor"], "=", err / c["floor"], "floors; bit-equal to the "
          "reference in", same, "; reprojection", px, "px")
    assert err <= 4 * c["floor"]
    assert px <= 0.01


def test_restatement_filter_order_and_records():
    """The restatement itself: stride grid, inclusive range ends, NaN and infinity dropped,
    (image, row, column) order, the colours of the kept pixels."""
    B, H, W = 2, 5, 7
    _, inv_K = pc.intrinsics(H, W, B)
    m = np.full((B, H, W), 10.0, np.float32)
    m[0, 0, 0], m[0, 0, 2], m[0, 2, 4], m[1, 4, 6] = np.nan, np.inf, 0.0, 80.0
    m[1, 0, 0], m[1, 0, 2] = np.nextafter(np.float32(80), np.float32(np.inf)), np.float32(1e-3)
    rgb = pc.colours(B, H, W, 1)
    rec, offsets, keep, _ = pc.points_np(m, rgb, inv_K, depth_input=True, stride=2)
    want = np.zeros((B, H, W), bool)
    want[:, ::2, ::2] = True
    want[0, 0, 0] = want[0, 0, 2] = want[0, 2, 4] = want[1, 0, 0] = False
    assert np.array_equal(keep, want) and offsets.tolist() == [0, 9, 20] and rec.size == 20
    b, y, x = np.nonzero(want)
    # the stored z is z * r_2, and the pseudo-inverse's third row is (0, 0, 1) only to an ulp
    assert np.allclose(rec["z"], m[b, y, x], rtol=1e-6, atol=0) and np.array_equal(rec["red"], rgb[b, y, x, 0])
    assert np.array_equal(rec["blue"], rgb[b, y, x, 2]) and rec.view(np.uint8).size == 15 * 20


def test_the_kernel_cases_are_what_they_claim():
    """The shapes the GPU tests run (tests/points_case.kernel_cases) do exercise what they are
    there for, according to the restatement."""
    cases = pc.kernel_cases

    @functools.lru_cache(maxsize=None)
    def expected(name):
        c = cases()[name]
        return pc.points_np(c["map"], c["rgb"], c["inv_K"], c["T"], **c["kw"])

    _, offsets, keep, _ = expected("mixed_3x37x50")
    assert [int(15 * int(o) % 4) for o in offsets[:-1]] == [0, 3, 3] and offsets[1] == offsets[2] == 925
    assert expected("1x1x1_kept")[1].tolist() == [0, 1] and expected("1x1x1_dropped")[1].tolist() == [0, 0]
    assert expected("stride64_3x37x50")[1].tolist() == [0, 1, 2, 3]
    for name in ("1x3x5", "row_65", "row_257", "row_1025", "col_1025", "stride2_3x37x50", "stride3_3x37x50",
                 "world_3x37x50", "2x64x128", "8200x1x1"):
        _, offsets, keep, _ = expected(name)
        grid = keep.shape[0] * len(range(0, keep.shape[1], cases()[name]["kw"].get("stride", 1))) * \
            len(range(0, keep.shape[2], cases()[name]["kw"].get("stride", 1)))
        assert 0 < offsets[-1] < grid, name                        # some kept, some dropped
    c = cases()["sparse_depth_2x37x50"]
    _, _, keep, _ = expected("sparse_depth_2x37x50")
    assert keep[0, 0, :4].tolist() == [True, False, True, False]    # near, below, above, negative
    assert keep[0, 36, 46:].tolist() == [True, False, True, False]  # far, above, below, infinite
    assert keep[1, 17, 20:24].tolist() == [True, True, False, False]
    assert not keep[c["map"] == 0].any() and 50 < keep.sum() < 400
    assert np.abs(cases()["world_3x37x50"]["T"][:, :3, 3]).max() > 100
