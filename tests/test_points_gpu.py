"""GPU tests of the point-cloud operator (csrc/points.hip, points_ops.depth_to_points) and
of the command (monodepth2_amd.pointcloud).

Yardsticks: tests/points_case.py, the numpy restatement of md2_depth_points in the kernel's
written order — the offsets and every record compared bytewise, the bytes behind the last
record against a sentinel — and tests/golden/points/points.npz, captured from the
reference's disp_to_depth and BackprojectDepth: the kernel's coordinates may lie 4 floors
from the recorded fp64 evaluation (torch's matmul rounds the same sum in another order; a
wrong term misses by orders of magnitude) and must reproject onto their pixel indices within
0.01 px.  Bitwise parity rests on nothing being contracted into an fma and on the device's
fp32 division being correctly rounded under the default compiler flags.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import points_case as pc
from monodepth2_amd import _lib
from monodepth2_amd import points_ops as po

pytestmark = pytest.mark.gpu

DEV = "cuda"
SENTINEL = 0xA5
CASES = list(pc.kernel_cases())


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@functools.lru_cache(maxsize=None)
def cases():
    return pc.kernel_cases()


@functools.lru_cache(maxsize=None)
def expected(name):
    """The restatement's (records, offsets, keep, coordinates) of a case: computed once, shared."""
    c = cases()[name]
    out = pc.points_np(c["map"], c["rgb"], c["inv_K"], c["T"], **c["kw"])
    for a in out:
        a.setflags(write=False)
    return out


def run_api(name, **extra):
    c = cases()[name]
    T = cuda(c["T"]) if c["T"] is not None else None
    return po.depth_to_points(cuda(c["map"]), cuda(c["rgb"]), cuda(c["inv_K"]), T, **c["kw"], **extra)


def run_raw(name, tail=64, misalign=0):
    """The C entry point on buffers of the test's own: `vertices` is filled with a sentinel,
    has `tail` spare bytes behind the capacity and starts `misalign` bytes off a dword."""
    c = cases()[name]
    B, H, W = c["map"].shape
    kw = dict(c["kw"])
    stride = kw.get("stride", 1)
    d = po.points_desc(B, H, W, world=c["T"] is not None, **kw)
    cap = po.capacity(B, H, W, stride)
    L = _lib.lib()
    ws = torch.full((L.md2_depth_points_workspace_bytes(ctypes.byref(d)),), 0x5A, dtype=torch.uint8, device=DEV)
    whole = torch.full((misalign + 15 * cap + tail,), SENTINEL, dtype=torch.uint8, device=DEV)
    vertices = whole[misalign:]
    offsets = torch.full((B + 1,), -1, dtype=torch.int32, device=DEV)
    m, rgb, inv_K = cuda(c["map"]), cuda(c["rgb"]), cuda(c["inv_K"])
    T = cuda(c["T"]) if c["T"] is not None else None
    _lib.check(L.md2_depth_points(ctypes.byref(d), m.data_ptr(), rgb.data_ptr(), inv_K.data_ptr(),
                                  T.data_ptr() if T is not None else None, vertices.data_ptr(), cap,
                                  offsets.data_ptr(), ws.data_ptr(), _lib.stream(torch.device(DEV, 0))),
               "md2_depth_points")
    torch.cuda.synchronize()
    return whole.cpu().numpy(), offsets.cpu().numpy().astype(np.uint32)


def check_bytes(name, whole, offsets, misalign=0):
    rec, want_offsets, _, _ = expected(name)
    assert np.array_equal(offsets, want_offsets), (name, offsets, want_offsets)
    n = int(want_offsets[-1])
    body = whole[misalign:misalign + 15 * n]
    got = np.frombuffer(body.tobytes(), pc.VERTEX)
    want_bytes = rec.view(np.uint8) if n else np.zeros(0, np.uint8)
    off = body != want_bytes
    if off.any():       # say what differs before failing: a coordinate one ulp off, or a misplaced record
        first = int(np.flatnonzero(off)[0]) // 15
        print(name, int(off.sum()), "bytes differ, first in record", first, "got", got[first], "want", rec[first])
    assert not off.any()
    assert (whole[:misalign] == SENTINEL).all() and (whole[misalign + 15 * n:] == SENTINEL).all()
    return n


@pytest.mark.parametrize("name", CASES)
def test_kernel_is_byte_equal_to_the_restatement(name):
    whole, offsets = run_raw(name)
    n = check_bytes(name, whole, offsets)
    print(name, "records", n, "image starts modulo 4", [int(15 * int(o) % 4) for o in offsets[:-1][:8]])
    vertices, api_offsets = run_api(name)
    c = cases()[name]
    B, H, W = c["map"].shape
    assert vertices.dtype == torch.uint8 and vertices.is_cuda
    assert vertices.numel() == 15 * po.capacity(B, H, W, c["kw"].get("stride", 1))
    assert api_offsets.shape == (B + 1,) and api_offsets.is_cuda
    assert np.array_equal(api_offsets.cpu().numpy().astype(np.uint32), offsets)
    assert np.array_equal(vertices[:15 * n].cpu().numpy(), whole[:15 * n])


@pytest.mark.parametrize("misalign", [1, 2, 3])
def test_a_vertex_buffer_off_a_dword_boundary(misalign):
    """`vertices` may start at any byte: the head and tail bytes follow the address."""
    whole, offsets = run_raw("mixed_3x37x50", misalign=misalign)
    check_bytes("mixed_3x37x50", whole, offsets, misalign)


def test_bitwise_repeatable_workspace_and_graph():
    name = "world_3x37x50"
    a = run_api(name)
    b = run_api(name)
    n = int(expected(name)[1][-1])
    assert torch.equal(a[1], b[1]) and torch.equal(a[0][:15 * n], b[0][:15 * n])
    need = po.workspace_bytes(3, 37, 50)
    ws = torch.full((need + 4096,), 0xFF, dtype=torch.uint8, device=DEV)       # garbage: no initialisation needed
    assert ws.data_ptr() % 256 == 0
    c_ = run_api(name, workspace=ws)
    assert torch.equal(a[1], c_[1]) and torch.equal(a[0][:15 * n], c_[0][:15 * n])
    with pytest.raises(ValueError, match="workspace"):
        run_api(name, workspace=ws[:need - 256] if need > 256 else ws[:0])
    # capturable: no allocation inside the operator when the workspace is the caller's
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run_api(name, workspace=ws)
    torch.cuda.current_stream().wait_stream(side)
    c = cases()[name]
    m, rgb, inv_K, T = cuda(c["map"]), cuda(c["rgb"]), cuda(c["inv_K"]), cuda(c["T"])
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = po.depth_to_points(m, rgb, inv_K, T, workspace=ws, **c["kw"])
    for _ in range(2):
        out[0].fill_(7), out[1].fill_(-1)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out[1], a[1]) and torch.equal(out[0][:15 * n], a[0][:15 * n])
        assert bool((out[0][15 * n:] == 7).all())


def test_input_checks():
    c = cases()["1x3x5"]
    m, rgb, k = cuda(c["map"]), cuda(c["rgb"]), cuda(c["inv_K"])
    v, o = po.depth_to_points(m[:, None], rgb, k, **c["kw"])                    # (B, 1, H, W) as well
    assert np.array_equal(o.cpu().numpy().astype(np.uint32), expected("1x3x5")[1])
    with pytest.raises(ValueError, match="float32"):
        po.depth_to_points(m.double(), rgb, k)
    with pytest.raises(ValueError, match="rgb"):
        po.depth_to_points(m, rgb[:, :, :, :2], k)
    with pytest.raises(ValueError, match="rgb"):
        po.depth_to_points(m, rgb.float(), k)
    with pytest.raises(ValueError, match="inv_K"):
        po.depth_to_points(m, rgb, k[:, :3, :3])
    with pytest.raises(ValueError, match="T must be"):
        po.depth_to_points(m, rgb, k, k[:, :3])
    with pytest.raises(RuntimeError, match="GPU only"):
        po.depth_to_points(m, rgb.cpu(), k)
    with pytest.raises(RuntimeError, match="near"):
        po.depth_to_points(m, rgb, k, near=0.0)


@pytest.mark.parametrize("name", list(pc.golden_cases()))
def test_coordinates_against_the_golden(name):
    """On the golden's inputs every pixel is kept (far is beyond the largest depth, 100): the
    kernel's coordinates within 4 floors of the recorded fp64 evaluation, and its records
    reprojected with K within 0.01 px of their pixel indices."""
    c = pc.case(pc.load_golden(), name)
    B, H, W = c["disp"].shape
    vertices, offsets = po.depth_to_points(cuda(c["disp"]), cuda(pc.colours(B, H, W, 0)), cuda(c["inv_K"]), far=1e4)
    assert offsets.cpu().numpy().tolist() == [H * W * b for b in range(B + 1)]
    rec = np.frombuffer(vertices.cpu().numpy().tobytes(), pc.VERTEX)
    P = np.stack([rec["x"], rec["y"], rec["z"]], 1).reshape(B, H, W, 3).transpose(0, 3, 1, 2).astype(np.float64)
    err = float((np.abs(P - c["f64"]).max(axis=1) / np.abs(c["f64"]).max(axis=1)).max())
    same = float((P.astype(np.float32).view(np.uint32) == c["cam"].view(np.uint32)).mean())
    u, v = pc.reproject_np(rec, c["K"][0])
    _, y, x = np.nonzero(np.ones((B, H, W), bool))
    px = float(max(np.abs(u - x).max(), np.abs(v - y).max()))
    print(name, "kernel vs fp64", err, "floor", c["floor"], "=", err / c["floor"], "floors; bit-equal to the "
          "reference in", same, "; reprojection", px, "px")
    assert err <= 4 * c["floor"]
    assert px <= 0.01


# ---- the command -------------------------------------------------------------------------

FEED = (64, 128)        # the smallest feed size the networks accept (tests/test_viz_gpu.py)


def picture(h, w, seed):
    rng = np.random.RandomState(seed)
    yy, xx = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    img = np.stack([(yy * 5 + xx * 3 + 40 * seed) % 256, (xx * 4 + 17) % 256, (yy * 6 + 90 * seed) % 256], 2)
    return np.clip(img + rng.randint(-12, 13, img.shape), 0, 255).astype(np.uint8)


@pytest.fixture(scope="module")
def demo(tmp_path_factory):
    """A random-weight ResNet-18 checkpoint with feed size 64 x 128, a folder with two lossless
    PNGs of different sizes and a folder with three of one size."""
    from PIL import Image
    from monodepth2_amd import networks
    root = tmp_path_factory.mktemp("pointcloud")
    torch.manual_seed(0)
    enc = networks.ResnetEncoder(18, False)
    dec = networks.DepthDecoder(enc.num_ch_enc)
    state = enc.state_dict()
    state["height"], state["width"], state["use_stereo"] = FEED[0], FEED[1], False
    (root / "weights").mkdir()
    torch.save(state, root / "weights" / "encoder.pth")
    torch.save(dec.state_dict(), root / "weights" / "depth.pth")
    (root / "mixed").mkdir()
    Image.fromarray(picture(37, 50, 1)).save(root / "mixed" / "a.png")
    Image.fromarray(picture(23, 41, 2)).save(root / "mixed" / "b.png")
    (root / "drive").mkdir()
    for i in range(3):
        Image.fromarray(picture(37, 50, 3 + i)).save(root / "drive" / ("%02d.png" % i))
    return root


@pytest.fixture
def recorded(monkeypatch):
    """The resized maps of the command's own passes: a second forward pass is not the
    yardstick (the eval-mode forward is not bitwise repeatable between passes)."""
    from monodepth2_amd import pointcloud as cmd
    calls = []

    def recording(disp, size, **kw):
        out = cmd_colorize(disp, size, **kw)
        calls.append((tuple(size), out[1].clone()))
        return out

    cmd_colorize = cmd.colorize_disparity
    monkeypatch.setattr(cmd, "colorize_disparity", recording)
    return calls


def cloud_of(resized, images, T=None, **kw):
    """depth_to_points and the restatement on recorded maps: the records, checked equal."""
    from monodepth2_amd import pointcloud as cmd
    n, H, W = resized.shape
    inv_K = np.repeat(cmd.inverse_intrinsics(cmd.DEFAULT_INTRINSICS, H, W)[None], n, 0)
    rgb = np.stack(images)
    vertices, offsets = po.depth_to_points(resized, cuda(rgb), cuda(inv_K), cuda(T) if T is not None else None, **kw)
    offsets = offsets.cpu().numpy().astype(np.uint32)
    rec = np.frombuffer(vertices[:15 * int(offsets[-1])].cpu().numpy().tobytes(), pc.VERTEX)
    want, want_offsets, _, _ = pc.points_np(resized.cpu().numpy(), rgb, inv_K, T, **kw)
    assert np.array_equal(offsets, want_offsets) and np.array_equal(rec.view(np.uint8), want.view(np.uint8))
    return rec, offsets


def test_command_writes_one_cloud_per_image(demo, recorded, capsys):
    from PIL import Image
    from monodepth2_amd import pointcloud as cmd
    images = demo / "mixed"
    cmd.main(["--image_path", str(images), "--load_weights_folder", str(demo / "weights"), "--ext", "png",
              "--stride", "2", "--far", "50"])
    text = capsys.readouterr().out
    assert "-> Making point clouds of 2 images" in text and "-> Done!" in text
    assert sorted(p.name for p in images.iterdir()) == ["a.png", "a_cloud.ply", "b.png", "b_cloud.ply"]
    assert [size for size, _ in recorded] == [(37, 50), (23, 41)]              # one operator call per size
    for (size, resized), name in zip(recorded, ("a", "b")):
        img = np.asarray(Image.open(images / (name + ".png")).convert("RGB"))
        assert resized.shape == (1,) + size and img.shape == size + (3,)
        rec, offsets = cloud_of(resized, [img], stride=2, far=50.0)
        got = po.read_ply(images / (name + "_cloud.ply"))
        print(name, "points", got.size, "of", len(range(0, size[0], 2)) * len(range(0, size[1], 2)))
        assert got.size == int(offsets[-1]) > 0
        assert np.array_equal(got.view(np.uint8), rec.view(np.uint8))


def test_command_fuses_a_drive_with_poses(demo, recorded, capsys):
    from PIL import Image
    from monodepth2_amd import pointcloud as cmd
    images = demo / "drive"
    poses = pc.rigid(2, 21, reach=1.5)
    np.save(demo / "poses.npy", poses)
    out = demo / "fused.ply"
    argv = ["--image_path", str(images), "--load_weights_folder", str(demo / "weights"), "--ext", "png"]
    cmd.main(argv + ["--poses", str(demo / "poses.npy"), "--out", str(out), "--pred_metric_depth"])
    assert "Fused 3 images" in capsys.readouterr().out
    assert sorted(p.name for p in images.iterdir()) == ["00.png", "01.png", "02.png"]   # one fused file, elsewhere
    assert len(recorded) == 1 and recorded[0][0] == (37, 50) and recorded[0][1].shape == (3, 37, 50)
    resized = recorded[0][1]
    imgs = [np.asarray(Image.open(images / ("%02d.png" % i)).convert("RGB")) for i in range(3)]
    chain = cmd.chain_poses(poses)
    rec, offsets = cloud_of(resized, imgs, chain, depth_scale=5.4)
    got = po.read_ply(out)
    assert got.size == int(offsets[-1]) == 3 * 37 * 50
    assert np.array_equal(got.view(np.uint8), rec.view(np.uint8))
    # block 0 (C_0 = I) is the first image's own cloud; block i is the operator with T = C_i
    own, _ = cloud_of(resized[:1], imgs[:1], depth_scale=5.4)
    assert np.array_equal(got[:offsets[1]].view(np.uint8), own.view(np.uint8))
    for i in (1, 2):
        block, _ = cloud_of(resized[i:i + 1], imgs[i:i + 1], chain[i:i + 1], depth_scale=5.4)
        assert np.array_equal(got[offsets[i]:offsets[i + 1]].view(np.uint8), block.view(np.uint8))
    assert not np.array_equal(got[offsets[1]:offsets[2]]["x"], cloud_of(resized[1:2], imgs[1:2], depth_scale=5.4)[0]["x"])
    # a wrong count is refused with both numbers, before the networks are loaded
    np.save(demo / "poses4.npy", pc.rigid(4, 22))
    with pytest.raises(SystemExit, match="holds 4 transforms but 3 images"):
        cmd.main(argv + ["--poses", str(demo / "poses4.npy"), "--out", str(out)])
