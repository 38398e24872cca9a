"""Which refusal wins when a call carries several invalid or mutually incompatible requests at once.

`_stabilize_frames` checks every keyword before it touches the clip or a GPU, in a fixed order; `stabilize_sharded` refuses
what it does not shard before it imports torch.distributed.  The single-feature tests pin each message; these tables pin the
ORDER: every call below is wrong in two or three ways and names the one message that is raised.  The messages were recorded
from the code as it stood before the checks moved into `FlowRequest` and the sharded refusals into a table."""

import numpy as np
import pytest


class NoClip:                      # never touched: the checks come first (len(None) would be a TypeError)
    frames = None


M = np.zeros((4, 4), np.float32)        # a mask whose shape is only looked at once the clip's length is known
M3 = np.zeros((2, 4, 4), np.float32)    # a subject mask of the [N,H,W] form (its N and size are checked later, too)

# (framing_mode, transform_mode, keywords, VSTAB_FLOW_BACKEND or None, the message that wins)
FLOW = [
    ("crop_and_pad", "similarity", dict(mask_tapered=False, dynamic_zoom=-1.0), None,
     'mask_tapered=False needs mask_grow, mask_feather or mask_hold: it chooses their footprint'),
    ("expand", "similarity", dict(dynamic_zoom=99.0, spatial_fill="yes"), None,
     'dynamic_zoom=99.0: expected None, True or a finite window in seconds in (0, 60]'),
    ("expand", "similarity", dict(dynamic_zoom=True, spatial_fill="yes"), None,
     "dynamic_zoom is not supported with framing_mode 'expand': an expand canvas has no frame to fill: it grows until it holds every frame. Use framing_mode 'crop_and_pad'."),
    ("crop_and_pad", "similarity", dict(spatial_fill="yes", stability_report=2, scene_cuts="sometimes"), None,
     "spatial_fill='yes' is not a bool (True fills the leftover padding, False leaves it)"),
    ("crop_and_pad", "similarity", dict(stability_report=2, scene_cuts="sometimes"), None,
     'stability_report=2 is not a bool (True adds the ITF of the inputs and of the outputs to the meta, False leaves it out)'),
    ("crop_and_pad", "similarity", dict(scene_cuts="sometimes", mesh_warp=(1, 1)), None,
     "scene_cuts='sometimes': expected None, 'auto' or a sequence of frame indices"),
    ("crop_and_pad", "similarity", dict(mesh_warp=(1, 1), mesh_motion=True, estimator="nope"), None,
     'mesh_warp=(1, 1): cols and rows must lie in [2, 64]'),
    ("crop_and_pad", "similarity", dict(mesh_motion=True, estimator="nope"), None,
     'mesh_motion=True needs mesh_warp: without a mesh warp there are no per-vertex offsets to record.'),
    ("crop_and_pad", "perspective", dict(estimator="nope", subject_mask=M, temporal_fill=99), None,
     "Unknown estimator 'nope'; expected 'flow' or 'classic'."),
    ("crop_and_pad", "perspective", dict(estimator="subject", subject_mask=M, temporal_fill=99), None,
     "transform_mode='perspective' is not supported with estimator 'subject': a centroid and an area determine no homography.  Use 'translation' or 'similarity'."),
    ("crop_and_pad", "similarity", dict(estimator="subject", temporal_fill=99), None,
     "estimator='subject' needs subject_mask: a float mask [N,H,W] of the subject, one per frame."),
    ("crop_and_pad", "similarity", dict(temporal_fill=99, fill_feather=8, sharpness_transfer=99), None,
     'temporal_fill=99 outside [0, 32]'),
    ("crop_and_pad", "similarity", dict(fill_feather=8, sharpness_transfer=99), None,
     'fill_feather=8 / fill_exposure=False need temporal_fill > 0: they change how the temporal fill writes its pixels'),
    ("crop_and_pad", "similarity", dict(fill_exposure=True, sharpness_transfer=2, mesh_warp=True), None,
     'fill_feather=None / fill_exposure=True need temporal_fill > 0: they change how the temporal fill writes its pixels'),
    ("crop_and_pad", "similarity", dict(sharpness_transfer=99, mesh_warp=True), None,
     'sharpness_transfer=99 is not 0, None, False or an integer in 1..16'),
    ("crop_and_pad", "similarity", dict(sharpness_transfer=2, mesh_warp=True, temporal_fill=2), None,
     'sharpness_transfer is not supported with mesh_warp: transfer candidates are global matrices, and a mesh-warped frame is not the image of its neighbours under one matrix'),
    ("crop_and_pad", "similarity", dict(sharpness_transfer=2, estimator="subject", subject_mask=M3, temporal_fill=2), None,
     "sharpness_transfer is not supported with estimator 'subject': its transitions are the subject's, not the camera's, so they do not register a neighbour's background"),
    ("crop_and_pad", "similarity", dict(estimator="classic", estimation_mask=M, mask_margin=99, mesh_warp=True), None,
     'mask_margin=99 outside [0, 64] (working pixels)'),
    ("crop_and_pad", "similarity", dict(estimator="classic", estimation_mask=M, mesh_warp=True), None,
     "estimation_mask is not supported with estimator 'classic': the Classic estimator fits tracked corners, not grid samples: it needs a masked corner detector, which does not exist yet."),
    ("crop", "similarity", dict(mesh_warp=True, temporal_fill=2, rolling_shutter=5.0), None,
     "mesh_warp is not supported with framing_mode 'crop': the crop solver bounds matrices only, so it cannot keep a per-vertex displacement free of padding."),
    ("crop_and_pad", "similarity", dict(mesh_warp=True, temporal_fill=2, rolling_shutter=0.5), None,
     'mesh_warp is not supported with temporal_fill=2: fill candidates are global matrices, which do not describe a mesh-warped neighbour.'),
    ("crop_and_pad", "similarity", dict(estimator="subject", subject_mask=M3, scene_cuts="auto"), None,
     "scene_cuts='auto' is not supported with estimator 'subject': the residual score is taken after the pair's camera transition, which this estimator does not measure.  Pass the cuts as a list of frame indices."),
    ("crop_and_pad", "similarity", dict(estimator="subject", subject_mask=M3, temporal_fill=2, rolling_shutter=0.5), None,
     "temporal_fill=2 is not supported with estimator 'subject': fill candidates register the background through the transitions, and these transitions are the subject's."),
    ("crop_and_pad", "similarity", dict(estimator="subject", subject_mask=M3, estimation_mask=M, rolling_shutter=7.0), None,
     "estimation_mask is not supported with estimator 'subject': the subject lock follows a mask's centroid: it has no camera-motion fit to keep a subject out of."),
    ("crop_and_pad", "similarity", dict(rolling_shutter=7.0, mesh_warp=True, mesh_motion=True), None,
     "rolling_shutter=7.0: expected None, 0, 'auto' or a finite readout in [-1, 1] (a fraction of the frame interval; negative: bottom to top)"),
    ("expand", "similarity", dict(rolling_shutter=0.5, dynamic_zoom=True), None,
     "dynamic_zoom is not supported with framing_mode 'expand': an expand canvas has no frame to fill: it grows until it holds every frame. Use framing_mode 'crop_and_pad'."),
    ("crop_and_pad", "perspective", dict(rolling_shutter="auto", dynamic_zoom=True, estimator="flow_phase_correlate"), None,
     "rolling_shutter is not supported with transform_mode 'perspective': the image velocity of a perspective transition is not affine, and the row correction is a closed form of an affine one."),
    ("crop_and_pad", "similarity", dict(rolling_shutter=0.5, sharpness_transfer=2, temporal_fill=2), None,
     'rolling_shutter is not supported with temporal_fill=2: fill candidates are neighbour frames that have not been corrected.'),
    ("crop_and_pad", "similarity", dict(sharpness_transfer=2, mesh_warp=True), "bogus",
     'sharpness_transfer is not supported with mesh_warp: transfer candidates are global matrices, and a mesh-warped frame is not the image of its neighbours under one matrix'),
    ("crop_and_pad", "similarity", dict(estimation_mask=M, mask_margin=99, rolling_shutter=7.0), "bogus",
     "VSTAB_FLOW_BACKEND='bogus': expected 'DIS' or 'phase_correlate' (TV-L1 needs opencv-contrib in the reference and is not provided)."),
    ("crop_and_pad", "similarity", dict(mask_grow=999, rolling_shutter=7.0, estimator="nope"), None,
     'mask_grow=999 is not None or an integer in -64..64'),
]

# (keywords of stabilize_sharded, the message that wins): each of the seven alone, adjacent pairs, and three at once
SHARDED = [
    (dict(estimator="subject", estimation_mask=M),
     "stabilize_sharded does not support estimator 'subject': the subject lock is not sharded (its mask is not distributed with each rank's frames); run the single-GPU pipeline for a subject lock"),
    (dict(estimation_mask=M, scene_cuts="auto"),
     "stabilize_sharded does not support estimation_mask: the sharded path does not distribute a mask with each rank's frames and halo; run the single-GPU pipeline for a masked estimation"),
    (dict(scene_cuts=[3], mesh_warp=True),
     'stabilize_sharded does not support scene_cuts: scene cuts are not sharded (the sharded plan treats the clip as one continuous camera move); run the single-GPU pipeline for a scene-aware stabilization'),
    (dict(mesh_warp=True, dynamic_zoom=True),
     "stabilize_sharded does not support mesh_warp: the mesh warp is not sharded (vertex paths need every rank's flow grid); run the single-GPU pipeline for a mesh-warped stabilization"),
    (dict(dynamic_zoom=2.0, rolling_shutter="auto"),
     "stabilize_sharded does not support dynamic_zoom: dynamic zoom is not sharded (the envelope needs every rank's extents); run the single-GPU pipeline for a dynamically zoomed stabilization"),
    (dict(rolling_shutter=0.5, sharpness_transfer=2),
     "stabilize_sharded does not support rolling_shutter=0.5: the rolling-shutter correction is not sharded (velocities and the readout estimate need every rank's transitions); run the single-GPU pipeline for it"),
    (dict(sharpness_transfer=2),
     'stabilize_sharded does not support sharpness_transfer=2: the sharpness transfer is not sharded (the sharded path holds no halo of neighbouring source frames); run the single-GPU pipeline for it'),
    (dict(estimator="subject"),
     "stabilize_sharded does not support estimator 'subject': the subject lock is not sharded (its mask is not distributed with each rank's frames); run the single-GPU pipeline for a subject lock"),
    (dict(estimation_mask=M),
     "stabilize_sharded does not support estimation_mask: the sharded path does not distribute a mask with each rank's frames and halo; run the single-GPU pipeline for a masked estimation"),
    (dict(scene_cuts="auto"),
     'stabilize_sharded does not support scene_cuts: scene cuts are not sharded (the sharded plan treats the clip as one continuous camera move); run the single-GPU pipeline for a scene-aware stabilization'),
    (dict(mesh_warp=(8, 8)),
     "stabilize_sharded does not support mesh_warp: the mesh warp is not sharded (vertex paths need every rank's flow grid); run the single-GPU pipeline for a mesh-warped stabilization"),
    (dict(dynamic_zoom=True),
     "stabilize_sharded does not support dynamic_zoom: dynamic zoom is not sharded (the envelope needs every rank's extents); run the single-GPU pipeline for a dynamically zoomed stabilization"),
    (dict(rolling_shutter="auto"),
     "stabilize_sharded does not support rolling_shutter='auto': the rolling-shutter correction is not sharded (velocities and the readout estimate need every rank's transitions); run the single-GPU pipeline for it"),
    (dict(sharpness_transfer=3, estimator="subject", rolling_shutter=0.25),
     "stabilize_sharded does not support estimator 'subject': the subject lock is not sharded (its mask is not distributed with each rank's frames); run the single-GPU pipeline for a subject lock"),
]


@pytest.mark.parametrize("case", range(len(FLOW)))
def test_the_first_refusal_in_the_fixed_order_wins(pkg, monkeypatch, case):
    from vstab_amd import flow_pipeline

    framing, mode, keywords, backend, message = FLOW[case]
    if backend is None:
        monkeypatch.delenv("VSTAB_FLOW_BACKEND", raising=False)
    else:
        monkeypatch.setenv("VSTAB_FLOW_BACKEND", backend)
    with pytest.raises(ValueError) as caught:
        flow_pipeline._stabilize_frames(NoClip(), framing, mode, True, 0.9, 0.8, 0.6, (127, 127, 127), 16.0, **keywords)
    assert str(caught.value) == message


@pytest.mark.parametrize("case", range(len(SHARDED)))
def test_sharded_refusals_come_in_their_order_before_any_process_group(pkg, case):
    """No context, no frames, no process group: the refusal is raised before any of them is looked at."""
    from vstab_amd import distributed

    keywords, message = SHARDED[case]
    with pytest.raises(ValueError) as caught:
        distributed.stabilize_sharded(None, None, 12, "crop_and_pad", "similarity", False, 0.7, 0.5, 0.6, (127, 127, 127), 16.0,
                                      **keywords)
    assert str(caught.value) == message
