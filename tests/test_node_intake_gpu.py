"""GPU: the post-warp nodes' shared intake (nodes.py: _device_frames, _stabilizer_mask, _check_clip_and_mask /
_place_socket_mask), for what only runs behind the GPU context; everything in front of it is pinned on the CPU by
tests/test_node_surface_cpu.py.

One Flow run of a small clip feeds all six mask-taking nodes.  However the same mask arrives -- on the device, on the host,
as an array, with a trailing axis, as a strided view, as one frame for the whole clip -- a node returns the same bits and
leaves every input as it was.
"""

import json
from types import SimpleNamespace

import numpy as np
import pytest

from tests.util import shake_path

pytestmark = pytest.mark.gpu

N, H, W = 6, 270, 480   # the size of test_temporal_fill_gpu._clip; the intake does not depend on it


def _bits(t):
    a = t.detach().cpu().numpy() if hasattr(t, "detach") else np.asarray(t)
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def run(pkg, ctx):
    """frames (device), and a crop_and_pad Flow node's stabilized frames, padding mask [N,H,W] and meta (host)."""
    import torch

    import bench
    from vstab_amd import nodes

    frames = bench.synth_clip(N, 0, H, W, torch.device("cuda"), mats=shake_path(N, W, H, "similarity", seed=3, amp=1.5))
    stabilized, mask, meta = nodes.VideoStabilizerFlow.execute(frames, 16.0, "crop_and_pad", "similarity", False, 0.9, 0.8, 0.6, "#7F7F7F")
    assert tuple(mask.shape) == (N, H, W) and mask.dtype == torch.float32 and 0 < float(mask.sum()) < mask.numel()
    return SimpleNamespace(nodes=nodes, frames=frames, stabilized=stabilized, mask=mask.cpu().contiguous(),
                           meta=json.loads(json.dumps(meta)))


# node -> its call with the mask in place; the first three take the stabilizer's own mask, the others any node's
CALLS = {
    "TemporalFill": lambda r, m: (r.frames, r.stabilized, m, r.meta, 4, "bilinear"),
    "SharpnessTransfer": lambda r, m: (r.frames, r.stabilized, r.meta, 2, 16.0, m),
    "Deflicker": lambda r, m: (r.frames, r.stabilized, m, r.meta, 1.0, "exposure"),
    "PaddingFill": lambda r, m: (r.stabilized, m),
    "StabilityReport": lambda r, m: (r.stabilized, m, r.frames),
    "CleanPlate": lambda r, m: (r.stabilized, m, True, 1, 0.1, 3),
}
SOCKET_FORM = ("PaddingFill", "StabilityReport", "CleanPlate")


def _execute(run, node, mask):
    """The node's outputs, after checking that no input tensor or array changed a bit."""
    args = CALLS[node](run, mask)
    before = [(a, _bits(a).copy()) for a in args if hasattr(a, "shape")]
    meta_before = json.dumps(run.meta, sort_keys=True)
    out = getattr(run.nodes, "VideoStabilizer" + node).execute(*args)
    for value, bits in before:
        assert np.array_equal(_bits(value), bits), f"{node} changed an input of shape {tuple(value.shape)}"
    assert json.dumps(run.meta, sort_keys=True) == meta_before
    return tuple(out)


def _assert_same(got, want, what):
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        if hasattr(w, "shape"):
            assert tuple(g.shape) == tuple(w.shape) and np.array_equal(_bits(g), _bits(w)), f"{what}: output {i} differs"
        else:
            assert g == w, f"{what}: output {i} differs"


def _strided(mask):
    """The same values as a view of every second column of a tensor twice as wide."""
    import torch

    wide = torch.zeros(mask.shape[:-1] + (2 * mask.shape[-1],), dtype=mask.dtype, device=mask.device)
    wide[..., ::2] = mask
    view = wide[..., ::2]
    assert not view.is_contiguous() and torch.equal(view, mask)
    return view


@pytest.mark.parametrize("node", list(CALLS))
def test_every_form_of_a_mask_gives_the_same_bits(run, node):
    mask = run.mask
    want = _execute(run, node, mask)                         # a contiguous float32 [N,H,W] host tensor
    forms = {"device tensor": mask.cuda(), "numpy array": mask.numpy(), "[N,H,W,1]": mask[..., None],
             "[N,H,W,1] on the device": mask.cuda()[..., None], "strided view": _strided(mask),
             "strided view on the device": _strided(mask.cuda())}
    for name, form in forms.items():
        _assert_same(_execute(run, node, form), want, f"{node}, mask as {name}")
    if node in SOCKET_FORM:                                  # one mask for the whole clip is its expansion
        one = mask[:1]
        want = _execute(run, node, one.expand(N, H, W).contiguous())
        for name, form in {"[1,H,W]": one, "[1,H,W] on the device": one.cuda(), "[1,H,W,1] array": one.numpy()[..., None],
                           "[1,H,W] expanded without a copy": one.cuda().expand(N, H, W)}.items():
            _assert_same(_execute(run, node, form), want, f"{node}, mask as {name}")


@pytest.mark.parametrize("node,who", [("TemporalFill", "temporal fill"), ("SharpnessTransfer", "sharpness transfer"),
                                      ("Deflicker", "deflicker")])
def test_stabilizers_mask_of_another_shape_is_refused(run, node, who):
    """The one refusal of these nodes that comes behind the context: the mask is compared with the frames on the device."""
    for wrong in (run.mask[:, :-1], run.mask[:-1].cuda(), run.mask.numpy()[:, :, 1:, None]):
        with pytest.raises(ValueError) as refusal:
            _execute(run, node, wrong)
        shape = tuple(wrong.shape[:3])
        assert str(refusal.value) == f"{who}: padding_mask {shape} does not match the stabilized frames {(N, H, W)}"


def test_value_range_rule_through_padding_fill(run):
    """A float clip in 0..255 is the clip its caller divided by 255 (float32, as numpy divides), bit for bit."""
    import torch

    clip255 = (run.stabilized * 255.0).contiguous()
    assert float(clip255.amax(dim=(1, 2, 3)).min()) > 1.5                     # every frame is taken for 0..255
    scaled = torch.from_numpy(clip255.numpy() / np.float32(255.0))
    want = _execute(SimpleNamespace(nodes=run.nodes, stabilized=scaled, meta=run.meta), "PaddingFill", run.mask)
    got = _execute(SimpleNamespace(nodes=run.nodes, stabilized=clip255, meta=run.meta), "PaddingFill", run.mask)
    _assert_same(got, want, "PaddingFill of a 0..255 clip")
    _assert_same(_execute(SimpleNamespace(nodes=run.nodes, stabilized=clip255.cuda(), meta=run.meta), "PaddingFill", run.mask), want,
                 "PaddingFill of a 0..255 clip on the device")
