"""GPU: vstab_track_template_batch (csrc/vstab_track.hip), the "track" estimator of the Flow pipeline and its node.

Everything the kernel returns is an integer and must equal the NumPy restatement (tests/track_restatement.py, whose
properties are checked on the CPU in tests/test_template_track_cpu.py) exactly: no tolerance anywhere in the kernel tests.
The end-to-end tests run on the restatement's analytic clip; the camera-lock bound is the one measured on the CPU there.
"""

import json

import numpy as np
import pytest

from tests import track_restatement as R
from tests.test_template_track_cpu import CENTRE_BOUND

pytestmark = pytest.mark.gpu


def _texture(n, h, w, seed, shifts=None):
    """u8 [n,h,w]: one random texture, smoothed a little, rolled by `shifts[k]` = (dx, dy) in frame k (default: a walk of up
    to +-2 px), plus noise of +-3 grey levels, so that costs are neither 0 nor tied."""
    rng = np.random.default_rng(seed)
    base = rng.integers(0, 256, (h + 64, w + 64)).astype(np.float64)
    base = (base + np.roll(base, 1, 0) + np.roll(base, 1, 1) + np.roll(base, (1, 1), (0, 1))) / 4.0
    if shifts is None:
        shifts = np.cumsum(rng.integers(-2, 3, (n, 2)), axis=0)
    out = np.empty((n, h, w), np.uint8)
    for k in range(n):
        dx, dy = int(shifts[k][0]), int(shifts[k][1])
        img = base[32 - dy:32 - dy + h, 32 - dx:32 - dx + w] + rng.integers(-3, 4, (h, w))
        out[k] = np.clip(img, 0, 255).astype(np.uint8)
    return out


def _run(ctx, gray, box, R_, key):
    import torch

    s = R.stride_of(box[2], box[3])
    d = torch.from_numpy(np.ascontiguousarray(gray)).to(ctx.device)
    keep = d.clone()
    tsums, pos, best, near, surface = ctx.track_template_batch(d, box, s, R_, key, want_surface=True)
    again = ctx.track_template_batch(d, box, s, R_, key)          # without the surface: the scratch slots carry the costs
    assert again[4] is None and torch.equal(d, keep)              # nothing is written to the input
    got = {"tsums": tsums.cpu().numpy(), "pos": pos.cpu().numpy(), "best": best.cpu().numpy().view(np.uint64),
           "near": near.cpu().numpy().view(np.uint64), "surface": surface.cpu().numpy().view(np.uint64)}
    for name, t in zip(("tsums", "pos", "best", "near"), again[:4]):
        a = t.cpu().numpy()
        assert np.array_equal(a.view(np.uint64) if a.dtype == np.int64 and name != "tsums" else a, got[name]), name
    return got, R.track(gray, box, s, R_, key)


def _assert_equal(got, want, what):
    for name in ("tsums", "pos", "best", "near", "surface"):
        assert got[name].shape == want[name].shape, (what, name)
        assert np.array_equal(got[name], want[name]), (what, name, np.argwhere(got[name] != want[name])[:4].tolist())


# (id, (n, h, w), box, R, key, seed)
CASES = [
    ("n1", (1, 29, 37), (5, 4, 12, 10), 24, 0, 1),                       # nothing is searched
    ("n2", (2, 29, 37), (5, 4, 12, 10), 5, 0, 2),
    ("n7_key0", (7, 67, 131), (40, 20, 24, 17), 6, 0, 3),
    ("n7_key3", (7, 67, 131), (40, 20, 24, 17), 6, 3, 3),                # both directions
    ("n7_key6", (7, 67, 131), (40, 20, 24, 17), 6, 6, 3),                # an empty forward direction
    ("box8x8", (4, 29, 37), (14, 10, 8, 8), 7, 1, 4),                    # the minimum box, stride 1
    ("box65x9_stride2", (3, 67, 131), (30, 25, 65, 9), 5, 1, 5),         # stride 2: 32 x 4 samples; 9 pixels >= 8, 4 samples are fine
    ("box130x70_stride3", (3, 96, 160), (12, 10, 130, 70), 4, 2, 6),     # stride 3: 43 x 23 samples
    ("edge_left_top", (3, 29, 37), (0, 0, 12, 10), 4, 0, 7),             # sentinel candidates on two sides
    ("edge_right_bottom", (3, 29, 37), (25, 19, 12, 10), 4, 2, 8),
    ("whole_frame", (3, 29, 37), (0, 0, 37, 29), 3, 0, 9),               # only (0, 0) is inside
    ("r1", (4, 29, 37), (10, 8, 12, 10), 1, 0, 10),
    ("r48_window_larger_than_frame", (3, 29, 37), (10, 8, 12, 10), 48, 1, 11),
]


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_kernel_equals_restatement(ctx, case):
    name, (n, h, w), box, R_, key, seed = case
    gray = _texture(n, h, w, seed)
    got, want = _run(ctx, gray, box, R_, key)
    _assert_equal(got, want, name)
    s = R.stride_of(box[2], box[3])
    assert got["tsums"][0] == (box[2] // s) * (box[3] // s)
    if name == "n1":
        assert got["pos"].tolist() == [[5, 4]] and got["best"].tolist() == [0] and got["surface"][0, 24, 24] == 0
        assert (got["surface"] == R.SENTINEL).sum() == 49 * 49 - 1 and (got["near"] == R.SENTINEL).sum() == 8
    if name == "whole_frame":
        assert got["pos"].tolist() == [[0, 0]] * 3
        assert ((got["surface"][1:] != R.SENTINEL).sum(axis=(1, 2)) == 1).all()
    if name.startswith("edge") or name.startswith("r48"):
        assert (got["surface"][[k for k in range(n) if k != key]] == R.SENTINEL).any()
    if name == "box65x9_stride2":
        assert s == 2 and got["tsums"][0] == 32 * 4
    if name == "box130x70_stride3":
        assert s == 3 and got["tsums"][0] == 43 * 23


def test_rows_staged_in_several_chunks(ctx):
    """A box of 640 x 640 pixels: stride 10, 64 x 64 samples, a staged row of 2R + 630 + 1 = 637 bytes, so the 32 KiB tile holds
    51 of the 64 template rows and the workgroup stages twice."""
    gray = _texture(2, 660, 700, 13, shifts=[(0, 0), (2, -1)])
    got, want = _run(ctx, gray, (20, 10, 640, 640), 3, 0)
    _assert_equal(got, want, "chunks")
    assert R.stride_of(640, 640) == 10 and got["tsums"][0] == 4096 and got["pos"].tolist() == [[20, 10], [22, 9]]


def test_a_constant_clip_stays_where_it_is(pkg, ctx):
    gray = np.full((4, 29, 37), 93, np.uint8)
    got, want = _run(ctx, gray, (10, 8, 12, 10), 6, 1)
    _assert_equal(got, want, "constant")
    assert got["pos"].tolist() == [[10, 8]] * 4 and got["best"].tolist() == [0] * 4     # every J is 0: the pick is (0, 0)
    inside = got["surface"] != R.SENTINEL
    assert (got["surface"][inside] == 0).all()
    frames = np.repeat((gray.astype(np.float32) / np.float32(255.0))[..., None], 3, axis=-1)
    with pytest.raises(ValueError, match="the box holds no texture"):
        _stabilize(ctx, frames, track_box=(10, 8, 12, 10), track_key=1)


def test_a_subject_that_leaves_the_frame(ctx):
    """The texture slides 5 px to the right per frame until the box's content is past the right edge.  The box follows it to
    the edge and is held there by the sentinel candidates beyond it.  Under the rule a frame cannot be all-sentinel: the chain
    starts inside the frame and a pick is never a sentinel candidate while (0, 0) is inside, so every start is inside --
    asserted here; the carried position of such a frame is therefore reached by no clip (the kernel's and the restatement's
    order give it (0, 0) all the same)."""
    n, h, w = 6, 29, 37
    gray = _texture(n, h, w, 14, shifts=[(5 * k, 0) for k in range(n)])
    got, want = _run(ctx, gray, (14, 9, 12, 10), 6, 0)
    _assert_equal(got, want, "leaving")
    assert got["pos"][:3].tolist() == [[14, 9], [19, 9], [24, 9]] and got["pos"][:, 0].max() <= w - 12
    assert (got["surface"][3:] == R.SENTINEL).any(axis=(1, 2)).all() and (got["best"] != R.SENTINEL).all()


# ---- end to end ----------------------------------------------------------------------------------------------------------
ARGS = (True, 1.0, 0.5, 0.6, (127, 127, 127), 16.0)      # camera_lock + strength 1
KEY = 0


def _stabilize(ctx, frames, estimator="track", **kw):
    import torch

    from vstab_amd import flow_pipeline as fp
    from vstab_amd import host_math as hm

    t = torch.from_numpy(np.ascontiguousarray(frames, dtype=np.float32)).to(ctx.device)
    return fp._stabilize_frames(hm._normalize_video_input(t), "crop_and_pad", "translation" if estimator == "track" else "similarity",
                                *ARGS, ctx=ctx, keep_on_device=True, estimator=estimator, **kw)


@pytest.fixture(scope="module")
def clip():
    gray, _ = R.analytic_clip()
    return np.repeat((gray.astype(np.float32) / np.float32(255.0))[..., None], 3, axis=-1)


@pytest.fixture(scope="module")
def locked(pkg, ctx, clip):
    return _stabilize(ctx, clip, track_box=R.analytic_box(KEY), track_key=KEY)


def _gray_of(ctx, frames):
    import torch

    t = torch.from_numpy(np.ascontiguousarray(frames, dtype=np.float32)).to(ctx.device)
    return ctx.gray_downscale(t, None).cpu().numpy()


def _block_of(gray, box, key, radius=24):
    from vstab_amd import template_track as tt

    size = (gray.shape[2], gray.shape[1])
    out = R.track(gray, box, R.stride_of(box[2], box[3]), radius, key)
    return tt.solve(out["tsums"], out["pos"], out["best"], out["near"], box, key, radius, box, size, size)[1]


def test_pipeline_positions_equal_the_restatement(pkg, ctx, clip, locked):
    block = locked.meta["template_track"]
    want = _block_of(_gray_of(ctx, clip), R.analytic_box(KEY), KEY)
    assert block["position"] == want["position"] and block["confidence"] == want["confidence"]
    assert block == want and block["lost"] == [] and block["version"] == 1 and block["samples"] == 40 * 32
    err = np.abs(np.array(block["position"]) - R.analytic_truth(KEY)).max()
    print("largest error of the tracked centre, px:", err)
    assert err <= CENTRE_BOUND
    assert locked.meta["flow_backend"] == "template_track" and locked.meta["motion_meta"]["source"] == "estimated_subject"
    assert locked.meta["transform_mode_applied"] == "translation" and not locked.device_plan["used"]
    assert json.loads(json.dumps(locked.meta)) == locked.meta


def test_camera_lock_holds_the_patch_still(pkg, ctx, clip, locked):
    """The restatement, run on the gray images of the OUTPUT frames from the box where the key frame's warp put it, finds the
    patch where frame `key` shows it, within the bound measured on the CPU (measured on an MI355X: 0.162 px)."""
    out = locked.frames.cpu().numpy()
    assert out.shape == clip.shape
    x, y, bw, bh = R.analytic_box(KEY)
    tx, ty = np.array(locked.meta["stabilization_warp"]["per_frame"][KEY]["applied_matrix"])[:2, 2]
    box = (x + int(round(tx)), y + int(round(ty)), bw, bh)               # (the patch is 3..4 px larger on every side)
    block = _block_of(_gray_of(ctx, out), box, KEY, radius=8)
    pos = np.array(block["position"])
    drift = np.abs(pos - pos[KEY]).max()
    print("largest deviation of the patch's centre in the locked frames, px:", drift, "smallest confidence:", min(block["confidence"]))
    assert block["lost"] == [] and drift <= CENTRE_BOUND


def test_the_default_path_is_untouched(pkg, ctx, clip):
    ctx.set_timing(True)
    try:
        import torch

        ctx.track_template_batch(torch.zeros((1, 16, 16), dtype=torch.uint8, device=ctx.device), (2, 2, 8, 8), 1, 2, 0)   # the kind exists
        ctx.set_timing(True)                             # clears the totals
        plain = _stabilize(ctx, clip, estimator="flow")
        off = _stabilize(ctx, clip, estimator="flow", track_box=None)
        assert ctx.kernel_ms_stats("track_template")[1] == 0                        # nothing new is launched
    finally:
        ctx.set_timing(False)
    bits = lambda t: t.cpu().numpy().view(np.uint32)
    assert np.array_equal(bits(plain.frames), bits(off.frames)) and np.array_equal(bits(plain.masks), bits(off.masks))
    assert json.dumps(plain.meta) == json.dumps(off.meta) and "template_track" not in off.meta
    with pytest.raises(ValueError, match="track_box=.* needs estimator='track', got estimator='flow'"):
        _stabilize(ctx, clip, estimator="flow", track_box=(1, 2, 30, 30))


def test_node(pkg, ctx, clip, locked):
    import torch

    from vstab_amd import nodes_track

    x, y, bw, bh = R.analytic_box(KEY)
    out = nodes_track.VideoStabilizerFlowTrack.execute(torch.from_numpy(clip), 16.0, "crop_and_pad", True, 1.0, 0.5, 0.6, "#7F7F7F",
                                                       x, y, bw, bh, KEY, 24)
    block = json.loads(json.dumps(out[2]))["template_track"]
    assert block == locked.meta["template_track"]
    assert np.array_equal(np.asarray(out[0].cpu()).view(np.uint32), locked.frames.cpu().numpy().view(np.uint32))
