"""ComfyUI V3 node classes and the extensions that list them.

The six nodes of the reference (NODE_CLASSES: Classic, Flow, Motion Apply, the two shake generators, Inverse) keep its socket
ids, order, defaults and output names (nodes/video_stabilizer_flow.py:643-763, nodes/video_stabilizer_motion_apply.py:29-129;
pinned by scripts/check_node_schema.py:28-64), so existing graphs keep working when this package replaces it.

The other 21 are this package's own, in three families:
- Flow variants (`_FlowVariant`): the Flow node plus the sockets of one `_stabilize_frames` feature.  A variant states its
  texts, its sockets and one function from their values to the keyword extras; the schema and `execute` are made from that.
  The two Motion Apply variants (`_ApplyVariant`) are stated the same way over `apply_motion`.
- Post-warp nodes (fills, sharpness transfer, deflicker, clean plate, stability report, mask grow), which take frames and
  masks in through one intake: `_device_frames`, `_stabilizer_mask`, `_check_clip_and_mask` / `_place_socket_mask`,
  `_check_clips_against_plan`.
- The extension classes, one per feature, made from the ordered table `_EXTENSION_CHAIN`.

tests/test_node_surface_cpu.py pins every schema, the registration, what each variant hands on and every refusal that
precedes the GPU work; DESIGN.md ("Adding a node") says how a new one is written.
"""

from __future__ import annotations

import inspect
import json
import os
from typing import Any

import numpy as np

from . import clean_plate, deflicker, host_math as hm, mask_handoff, native, scene_cuts, sharpness_transfer, spatial_fill
from . import stability, temporal_fill
from .apply_pipeline import apply_motion
from .meta_v2 import resolve_motion_meta
from .comfy_compat import ComfyExtension, ProgressBar, io
from .dynamic_zoom import DEFAULT_WINDOW_S, DEFAULT_ZOOM_LIMIT, WINDOW_MAX_S, ZOOM_LIMIT_MAX, ZOOM_LIMIT_MIN
from .flow_pipeline import _fps_fields, _stabilize_frames
from .horizon_level import DEFAULT_LIMIT_DEG, LIMIT_MAX_DEG, WINDOW_MAX_S as LEVEL_WINDOW_MAX_S
from .mesh_warp import CELLS_MAX, CELLS_MIN, DEFAULT_CELLS
from .shake_generator import FIELD_RANGE, STYLES, ShakeRecipe, generate_shake_motion_meta

JSONType = io.Custom("JSON")

BLUR_QUALITY_SAMPLES = {"Draft": 5, "Standard": 9, "High": 17, "Ultra": 33}  # motion_apply node :21-26


def _keep_on_device() -> bool:
    """with VSTAB_KEEP_ON_DEVICE=1 the IMAGE / MASK outputs stay in HBM (torch device tensors), so a
    Flow -> Motion Apply chain avoids the 15 GB host round trip of a 256x1080p clip.  Default: CPU tensors, as
    the reference returns (stabilizer_utils.py:200-221)."""
    return os.environ.get("VSTAB_KEEP_ON_DEVICE", "0") not in ("", "0", "false", "False")


def _image_out(frames, context):
    if _keep_on_device() and hasattr(frames, "device") and context.template_kind != "dict":
        return frames
    return hm._reconstruct_video(frames, context)


def _mask_out(masks, levels: int = 1):
    """levels: the motion-blur samples S behind a soft mask (its values are 1 - c / S: they may cross PCIe as bytes), 1 otherwise."""
    if _keep_on_device() and hasattr(masks, "device"):
        return masks[..., 0] if masks.ndim == 4 else masks
    return hm._convert_masks_for_output(masks, levels)


def _estimator_inputs(transform_tip: str, lock_tip: str, framing_tip: str, strength_tip: str, smooth_tip: str) -> list:
    """The nine input sockets shared by the Flow and Classic nodes (flow.py:657-726, classic.py:586-659):
    same ids, order, defaults and ranges; only some tooltips differ."""
    slider = io.NumberDisplay.slider
    return [
        io.Image.Input("frames", display_name="Frames"),
        io.Float.Input("frame_rate", default=16.0, min=1.0, step=0.1, display_name="Input FPS",
                       tooltip="Frame rate in frames per second used to scale smoothing window."),
        io.Combo.Input("framing_mode", options=["crop", "crop_and_pad", "expand"], default="crop_and_pad",
                       display_name="Framing Mode", tooltip=framing_tip),
        io.Combo.Input("transform_mode", options=["translation", "similarity", "perspective"],
                       default="similarity", display_name="Transform Mode", tooltip=transform_tip),
        io.Boolean.Input("camera_lock", default=False, display_name="Camera Lock", tooltip=lock_tip),
        io.Float.Input("strength", default=0.7, min=0.0, max=1.0, step=0.05, display_name="Strength",
                       tooltip=strength_tip, display_mode=slider),
        io.Float.Input("smooth", default=0.5, min=0.0, max=1.0, step=0.05, display_name="Smooth",
                       tooltip=smooth_tip, display_mode=slider),
        io.Float.Input("keep_fov", default=0.6, min=0.0, max=1.0, step=0.05, display_name="Keep FOV",
                       tooltip=("[Crop only] How much of the original FOV to preserve (1.0 = no zoom, 0.0 = maximum "
                                "zoom). Ignored when framing_mode is crop_and_pad or expand."),
                       display_mode=slider),
        io.Color.Input("padding_color", default="#7F7F7F", display_name="Padding Color",
                       tooltip="HEX padding color applied in crop_and_pad / expand (e.g. #404040)."),
    ]


def _schema(node_id: str, display_name: str, description: str, **extra) -> io.Schema:
    """The shell of every node's schema; define_schema fills in `inputs` and `outputs`, with fresh sockets on every call."""
    return io.Schema(node_id=node_id, display_name=display_name, category="Video/Stabilization", description=description, **extra)


def _estimator_outputs() -> list:
    return [
        io.Image.Output("frames_stabilized", display_name="Stabilized Frames"),
        io.Mask.Output("padding_mask", display_name="Padding Mask"),
        JSONType.Output("meta", display_name="Motion Meta"),
    ]


def _clip_outputs() -> list:
    """Frames, padding mask and meta, as Motion Apply names them."""
    return [
        io.Image.Output("frames", display_name="Frames"),
        io.Mask.Output("padding_mask", display_name="Padding Mask"),
        JSONType.Output("meta", display_name="Meta"),
    ]


def _run_estimator_node(estimator: str, frames: Any, frame_rate: float, framing_mode: str, transform_mode: str,
                        camera_lock: bool, strength: float, smooth: float, keep_fov: float, padding_color: str, **extras):
    """What every estimator node's `execute` does; extras: the keyword extras of _stabilize_frames a Flow variant adds."""
    context = hm._normalize_video_input(frames)
    result = _stabilize_frames(
        context, framing_mode, transform_mode, camera_lock, strength, smooth, keep_fov,
        hm._parse_padding_color(padding_color), frame_rate, keep_on_device=True, estimator=estimator, **extras,
    )
    return io.NodeOutput(_image_out(result.frames, context), _mask_out(result.masks), result.meta)


class VideoStabilizerFlow(io.ComfyNode):
    """Dense-flow (DIS) stabilizer; all pixel work runs on the MI355X through libvstab."""

    @classmethod
    def define_schema(cls) -> io.Schema:
        schema = _schema("video_stabilizer_flow", "Video Stabilizer Flow",
                         description=("Video stabilization using dense optical flow with configurable transforms and framing, "
                                      "emitting stabilized frames, a padding mask, and motion diagnostics (MI355X build)."))
        schema.inputs = _estimator_inputs(
            transform_tip="Select the geometric model fitted to the optical flow.",
            lock_tip="Aggressively pull the motion curve toward a locked tripod-like solution.",
            framing_tip="Choose how borders produced by stabilization are handled.",
            strength_tip="Removal gain (0 keeps original motion, 1 removes it using the smoothed motion curve).",
            smooth_tip="Temporal smoothing amount applied to the motion curve before removal.",
        )
        schema.outputs = _estimator_outputs()
        return schema

    @classmethod
    def execute(cls, frames: Any, frame_rate: float, framing_mode: str, transform_mode: str, camera_lock: bool,
                strength: float, smooth: float, keep_fov: float, padding_color: str) -> io.NodeOutput:
        return _run_estimator_node("flow", frames, frame_rate, framing_mode, transform_mode, camera_lock, strength,
                                   smooth, keep_fov, padding_color)


class VideoStabilizerClassic(io.ComfyNode):
    """Sparse feature-tracking stabilizer (corner detection + pyramidal LK, classic.py:69-160) -- same sockets
    and meta as the reference's `Video Stabilizer Classic`; the tracker runs on the MI355X as well."""

    @classmethod
    def define_schema(cls) -> io.Schema:
        schema = _schema("video_stabilizer_classic", "Video Stabilizer Classic",
                         description=("Video stabilization using sparse feature tracking with configurable transforms and framing, "
                                      "emitting both stabilized frames and a padding mask (MI355X build)."))
        schema.inputs = _estimator_inputs(
            transform_tip="Select the geometric model used to estimate camera motion.",
            lock_tip="Treat the shot as tripod-like by aggressively damping motion.",
            framing_tip="Choose how to handle borders produced by stabilization.",
            strength_tip="Removal gain (0 keeps original motion, 1 removes it based on smoothing).",
            smooth_tip="Temporal smoothing amount applied to the estimated motion path.",
        )
        schema.outputs = _estimator_outputs()
        return schema

    @classmethod
    def execute(cls, frames: Any, frame_rate: float, framing_mode: str, transform_mode: str, camera_lock: bool,
                strength: float, smooth: float, keep_fov: float, padding_color: str) -> io.NodeOutput:
        return _run_estimator_node("classic", frames, frame_rate, framing_mode, transform_mode, camera_lock, strength,
                                   smooth, keep_fov, padding_color)


class VideoStabilizerMotionApply(io.ComfyNode):
    """Apply motion_meta matrices (optionally with matrix-sampled motion blur) to a clip."""

    @classmethod
    def define_schema(cls) -> io.Schema:
        schema = _schema("video_stabilizer_motion_apply", "Video Stabilizer Motion Apply",
                         description="Applies motion metadata to frames and emits a padding mask.")
        schema.inputs = [
            io.Image.Input("frames", display_name="Frames"),
            JSONType.Input("motion_meta", display_name="Motion Meta"),
            io.Combo.Input("framing_mode", options=["crop_and_pad", "crop", "expand"], default="crop_and_pad",
                           display_name="Framing Mode"),
            io.Combo.Input("interpolation", options=["bilinear", "bicubic"], default="bilinear",
                           display_name="Interpolation"),
            io.Color.Input("padding_color", default="#7F7F7F", display_name="Padding Color",
                           tooltip="HEX padding color used where warping exposes empty pixels."),
            io.Float.Input("motion_blur", default=0.0, min=0.0, max=1.0, step=0.05, display_name="Motion Blur",
                           tooltip="Shutter fraction for matrix-sampled motion blur. 0 disables blur.",
                           display_mode=io.NumberDisplay.slider),
            io.Combo.Input("motion_blur_quality", options=list(BLUR_QUALITY_SAMPLES.keys()), default="Standard",
                           display_name="Blur Quality",
                           tooltip="Draft is faster. High and Ultra average more shutter samples for smoother blur."),
        ]
        schema.outputs = _clip_outputs()
        return schema

    @classmethod
    def execute(cls, frames: Any, motion_meta: dict, framing_mode: str, interpolation: str, padding_color: str,
                motion_blur: float, motion_blur_quality: str) -> io.NodeOutput:
        context = hm._normalize_video_input(frames)
        quality = motion_blur_quality if motion_blur_quality in BLUR_QUALITY_SAMPLES else "Standard"
        samples = BLUR_QUALITY_SAMPLES[quality]
        n = len(context.frames)
        per_frame = int(max(3, min(33, samples))) if motion_blur > 0.0 else 1
        total = max(n * per_frame + (n if framing_mode == "crop" else 0), 1)
        pbar = ProgressBar(total)
        done = 0

        def tick() -> None:
            nonlocal done
            done += 1
            pbar.update_absolute(min(done, total), total)

        result = apply_motion(context, motion_meta, hm._parse_padding_color(padding_color),
                              framing_mode=framing_mode, interpolation=interpolation, motion_blur=motion_blur,
                              motion_blur_samples=samples, progress_callback=tick, keep_on_device=True)
        result.meta.setdefault("motion_apply", {})["motion_blur_quality"] = quality
        pbar.update_absolute(total, total)
        ma = result.meta.get("motion_apply", {})
        levels = int(ma.get("motion_blur_samples", 1)) if float(ma.get("motion_blur", 0.0)) > 0.0 else 1
        return io.NodeOutput(_image_out(result.frames, context), _mask_out(result.masks, levels), result.meta)


class VideoStabilizerInverse(io.ComfyNode):
    """Deprecated thin wrapper kept for graph compatibility (nodes/video_stabilizer_inverse.py:26-93 of the
    reference): inverse of the recorded stabilization warp through Motion Apply (crop_and_pad, bilinear)."""

    @classmethod
    def define_schema(cls) -> io.Schema:
        schema = _schema("video_stabilizer_inverse", "Video Stabilizer Inverse",
                         description=("Deprecated: use Video Stabilizer Motion Apply. Restores stabilized frames to the original "
                                      "canvas using stabilization metadata, and emits a padding mask for areas without source pixels."), is_deprecated=True)
        schema.inputs = [
            io.Image.Input("frames", display_name="Frames"),
            JSONType.Input("meta", display_name="Meta"),
            io.Color.Input("padding_color", default="#7F7F7F", display_name="Padding Color",
                           tooltip="HEX padding color used where inverse warping exposes empty pixels."),
        ]
        schema.outputs = [
            io.Image.Output("frames_restored", display_name="Restored Frames"),
            io.Mask.Output("padding_mask", display_name="Padding Mask"),
            JSONType.Output("meta", display_name="Meta"),
        ]
        return schema

    @classmethod
    def execute(cls, frames: Any, meta: dict, padding_color: str) -> io.NodeOutput:
        context = hm._normalize_video_input(frames)
        legacy = dict(meta)
        legacy.pop("motion_meta", None)   # force the inverse of stabilization_warp
        motion = resolve_motion_meta(legacy)
        result = apply_motion(context, legacy, hm._parse_padding_color(padding_color), framing_mode="crop_and_pad",
                              interpolation="bilinear", keep_on_device=True)
        if isinstance(meta, dict) and isinstance(meta.get("motion_meta"), dict):
            result.meta["motion_meta"] = meta["motion_meta"]
        result.meta.pop("motion_apply", None)
        warp = meta.get("stabilization_warp", {}) if isinstance(meta, dict) else {}
        result.meta["inverse_stabilization"] = {
            "source_size": [int(motion.output_size[0]), int(motion.output_size[1])],
            "input_size": [int(motion.input_size[0]), int(motion.input_size[1])],
            "output_size": [int(motion.output_size[0]), int(motion.output_size[1])],
            "matrix_convention": "stabilized_to_source",
            "source_matrix_convention": "source_to_stabilized",
            "framing_mode": warp.get("framing_mode") if isinstance(warp, dict) else None,
            "note": "Restores original motion/canvas; pixels discarded by crop framing cannot be recovered.",
        }
        return io.NodeOutput(_image_out(result.frames, context), _mask_out(result.masks), result.meta)


def _shake_common_inputs(middle: list) -> list:
    """`frames_context`, `frame_rate`, <node-specific sockets>, `amount`, `speed`, `seed`
    (video_stabilizer_shake_generator.py:27-79, video_stabilizer_shake_generator_manual.py:29-136)."""
    slider = io.NumberDisplay.slider
    return [
        io.Image.Input("frames_context", display_name="Frames Context",
                       tooltip=("The input frames are used only to read frame count and resolution. This node outputs "
                                "motion metadata only; connect it to Video Stabilizer Motion Apply to move pixels.")),
        io.Float.Input("frame_rate", default=16.0, min=1.0, step=0.1, display_name="Input FPS",
                       tooltip="Fallback frame rate when the input does not carry fps metadata."),
        *middle,
        io.Float.Input("amount", default=1.0, min=0.0, max=3.0, step=0.05, display_name="Amount", display_mode=slider),
        io.Float.Input("speed", default=1.0, min=0.1, max=3.0, step=0.05, display_name="Speed", display_mode=slider),
        io.Int.Input("seed", default=0, min=0, max=0xFFFFFFFFFFFFFFFF, display_name="Seed",
                     control_after_generate=io.ControlAfterGenerate.fixed),
    ]


def _shake_block(frames_context: Any, frame_rate: float, recipe: ShakeRecipe, amount: float, speed: float, seed: int,
                 node: str, style: str):
    context = hm._normalize_video_input(frames_context)   # only frame count and size are read; pixels are untouched
    block = generate_shake_motion_meta(recipe=recipe, frame_count=len(context.frames), width=context.width,
                                       height=context.height, fps=hm._resolve_fps(context, frame_rate), amount=amount,
                                       speed=speed, seed=seed, node=node, style=style)
    return io.NodeOutput({"motion_meta": block})


class VideoStabilizerShakeGenerator(io.ComfyNode):
    """Deterministic synthetic camera shake by style preset -> motion_meta (host only, no pixels)."""

    @classmethod
    def define_schema(cls) -> io.Schema:
        schema = _schema("video_stabilizer_shake_generator", "Video Stabilizer Shake Generator",
                         description="Generates deterministic shake motion metadata; it does not alter input frames.")
        schema.inputs = _shake_common_inputs([
            io.Combo.Input("style", options=list(STYLES.keys()), default="handheld", display_name="Style")])
        schema.outputs = [JSONType.Output("motion_meta", display_name="Motion Meta")]
        return schema

    @classmethod
    def execute(cls, frames_context: Any, frame_rate: float, style: str, amount: float, speed: float, seed: int) -> io.NodeOutput:
        return _shake_block(frames_context, frame_rate, STYLES[style], amount, speed, seed, "shake_generator", style)


_MANUAL_FIELDS = [  # id, step, display name (ranges come from shake_generator.FIELD_RANGE, defaults from the handheld preset)
    ("pan", 0.01, "Pan"), ("tilt", 0.01, "Tilt"), ("roll", 0.01, "Roll"), ("zoom", 0.001, "Zoom"),
    ("drift_freq", 0.05, "Drift Frequency"), ("tremor", 0.05, "Tremor"), ("tremor_freq", 0.5, "Tremor Frequency"),
    ("jitter_rate", 0.1, "Jitter Rate"), ("step", 0.05, "Step"), ("randomness", 0.05, "Randomness"),
    ("virtual_fov", 1.0, "Virtual FOV"),
]


class VideoStabilizerShakeGeneratorManual(io.ComfyNode):
    """The same generator driven by explicit recipe values."""

    @classmethod
    def define_schema(cls) -> io.Schema:
        schema = _schema("video_stabilizer_shake_generator_manual", "Video Stabilizer Shake Generator Manual",
                         description="Generates deterministic shake motion metadata from manual absolute values.")
        base = STYLES["handheld"]
        fields = []
        for name, step, label in _MANUAL_FIELDS:
            extra = {"display_mode": io.NumberDisplay.slider} if name == "randomness" else {}
            fields.append(io.Float.Input(name, default=getattr(base, name), min=FIELD_RANGE[name][0], max=FIELD_RANGE[name][1],
                                         step=step, display_name=label, **extra))
        schema.inputs = _shake_common_inputs(fields)
        schema.outputs = [JSONType.Output("motion_meta", display_name="Motion Meta")]
        return schema

    @classmethod
    def execute(cls, frames_context: Any, frame_rate: float, pan: float, tilt: float, roll: float, zoom: float,
                drift_freq: float, tremor: float, tremor_freq: float, jitter_rate: float, step: float, randomness: float,
                virtual_fov: float, amount: float, speed: float, seed: int) -> io.NodeOutput:
        recipe = ShakeRecipe(pan, tilt, roll, zoom, drift_freq, tremor, tremor_freq, jitter_rate, step, randomness, virtual_fov)
        return _shake_block(frames_context, frame_rate, recipe, amount, speed, seed, "shake_generator_manual", "manual")


# ---- the post-warp nodes' intake: who = the node's message prefix ("temporal fill", "padding fill", ...)

def _device_frames(video, ctx):
    """A clip's frames on the device under F0's value-range rule, as the stabilizer applies it: a float frame whose peak exceeds
    1.5 is 0..255 and is divided by 255."""
    batch = video.device_batch(ctx)
    if video.range_pending and hm.resolve_value_range(video, hm.prefetch_peaks(ctx.frame_range(batch)), ctx):
        batch = video.device_batch(ctx)
    return batch


def _check_clips_against_plan(who: str, plan: dict, context, out_context) -> None:
    """The original and the stabilized clip against temporal_fill.plan_from_meta: frame count, then source -> output size."""
    n = len(plan["final_matrices"])
    if len(context.frames) != n or len(out_context.frames) != n:
        raise ValueError(f"{who}: meta describes {n} frames, got {len(context.frames)} original and "
                         f"{len(out_context.frames)} stabilized frames")
    if (context.width, context.height) != plan["source_size"] or (out_context.width, out_context.height) != plan["output_size"]:
        raise ValueError(f"{who}: frame sizes {(context.width, context.height)} -> "
                         f"{(out_context.width, out_context.height)} do not match the meta's "
                         f"{plan['source_size']} -> {plan['output_size']}")


def _stabilizer_mask(who: str, padding_mask: Any, dst, ctx, copy: bool = False):
    """The stabilizer's own padding mask (a tensor or an array, [N,H,W] or [N,H,W,1]) as a contiguous float32 device tensor of
    the stabilized frames' shape, which is all it may have.  copy: a private one, for a node that writes the mask -- the
    caller's tensor (another node's cached output) stays as it is."""
    torch = ctx.torch
    mask = padding_mask if isinstance(padding_mask, torch.Tensor) else torch.from_numpy(np.asarray(padding_mask, dtype=np.float32))
    mask = mask.to(device=ctx.device, dtype=torch.float32)
    if mask.ndim == 4:
        mask = mask[..., 0]
    if tuple(mask.shape) != tuple(dst.shape[:3]):
        raise ValueError(f"{who}: padding_mask {tuple(mask.shape)} does not match the stabilized frames {tuple(dst.shape[:3])}")
    mask = mask.contiguous()
    return mask.clone() if copy else mask


def _check_clip_and_mask(who: str, context, padding_mask: Any, optional: bool = True):
    """The checks of a `frames` / `padding_mask` socket pair, all before any GPU work: the mask of any node, [N,H,W], [1,H,W] for
    every frame, or either with a trailing axis of 1.  -> (n, h, w), the mask's leading size (None without a mask)."""
    n, h, w = len(context.frames), context.height, context.width
    if n == 0:
        raise ValueError(f"{who}: socket 'frames' holds no frame")
    if padding_mask is None and optional:
        return (n, h, w), None
    if not (hasattr(padding_mask, "dtype") and hasattr(padding_mask, "shape")):
        raise ValueError(f"{who}: socket 'padding_mask' must be a floating-point MASK tensor, got {type(padding_mask).__name__}")
    if "float" not in str(padding_mask.dtype):
        raise ValueError(f"{who}: socket 'padding_mask' must be a floating-point MASK, got {padding_mask.dtype}")
    shape = tuple(int(v) for v in padding_mask.shape)
    if len(shape) == 4 and shape[3] == 1:
        shape = shape[:3]
    if len(shape) != 3 or shape[1:] != (h, w) or shape[0] not in (1, n):
        raise ValueError(f"{who}: socket 'padding_mask' of shape {tuple(padding_mask.shape)} does not match socket "
                         f"'frames' [{n},{h},{w},3]: expected [{n},{h},{w}] or [1,{h},{w}]")
    return (n, h, w), shape[0]


def _place_socket_mask(padding_mask: Any, lead: int, dims, ctx, copy: bool = False):
    """A mask that passed _check_clip_and_mask as a float32 [N,H,W] device tensor (None without a mask).  copy: a private one,
    for a node that writes the mask; otherwise a mask that is already in place is handed on as it is."""
    if lead is None:
        return None
    torch = ctx.torch
    mask = padding_mask if isinstance(padding_mask, torch.Tensor) else torch.from_numpy(np.asarray(padding_mask))
    mask = mask.to(device=ctx.device, dtype=torch.float32).reshape((lead,) + tuple(dims[1:])).expand(*dims)
    return mask.clone() if copy else mask.contiguous()


class VideoStabilizerTemporalFill(io.ComfyNode):
    """Fills the padding of a Flow / Classic result from neighbouring frames (temporal_fill.py), from the meta JSON alone:
    `stabilization_warp` gives the applied matrices, `estimated_motion.per_transition` the frame-to-frame motion.  Not one
    of the reference's nodes: it is registered by the extension but kept out of NODE_CLASSES."""

    @classmethod
    def define_schema(cls) -> io.Schema:
        schema = _schema("video_stabilizer_temporal_fill", "Video Stabilizer Temporal Fill",
                         description=("Fills padded pixels of stabilized frames with what neighbouring frames saw there, using the "
                                      "stabilizer's own motion metadata; the remaining mask marks what no frame within the radius saw."))
        schema.inputs = [
            io.Image.Input("frames", display_name="Frames", tooltip="The original (unstabilized) frames."),
            io.Image.Input("frames_stabilized", display_name="Stabilized Frames"),
            io.Mask.Input("padding_mask", display_name="Padding Mask"),
            JSONType.Input("meta", display_name="Motion Meta"),
            io.Int.Input("radius", default=8, min=1, max=32, display_name="Radius",
                         tooltip="Frames before and after each frame that may supply its missing pixels."),
            io.Combo.Input("interpolation", options=["bilinear", "bicubic"], default="bilinear", display_name="Interpolation"),
        ]
        schema.outputs = _clip_outputs()
        return schema

    @classmethod
    def execute(cls, frames: Any, frames_stabilized: Any, padding_mask: Any, meta: dict, radius: int,
                interpolation: str) -> io.NodeOutput:
        return cls._fill(frames, frames_stabilized, padding_mask, meta, radius, interpolation)

    @classmethod
    def _fill(cls, frames: Any, frames_stabilized: Any, padding_mask: Any, meta: dict, radius: int, interpolation: str,
              feather=None, exposure: bool = False) -> io.NodeOutput:
        """The node's work; feather / exposure are the blended node's two sockets (None / False: the plain fill)."""
        plan = temporal_fill.plan_from_meta(meta)   # ValueError naming the missing key, before any GPU work
        feather, exposure = temporal_fill.check_blend_request(int(radius), feather, exposure)
        if interpolation not in native.INTERP:
            raise ValueError(f"Unknown interpolation {interpolation!r}; expected 'bilinear' or 'bicubic'.")
        context = hm._normalize_video_input(frames)
        out_context = hm._normalize_video_input(frames_stabilized)
        _check_clips_against_plan("temporal fill", plan, context, out_context)
        ctx = native.default_context()
        src = _device_frames(context, ctx)
        # the fill works in place: on copies, so the caller's tensors (another node's cached outputs) stay as they are
        dst = out_context.device_batch(ctx).clone()
        mask = _stabilizer_mask("temporal fill", padding_mask, dst, ctx, copy=True)
        block = temporal_fill.fill_on_device(ctx, src, dst, mask, plan["final_matrices"], plan["transitions"],
                                             plan["confidences"], int(radius), interp=interpolation, feather=feather,
                                             exposure=exposure)
        block["interpolation"] = interpolation
        out_meta = dict(meta)
        out_meta["temporal_fill"] = block
        return io.NodeOutput(_image_out(dst, out_context), _mask_out(mask), out_meta)


class VideoStabilizerTemporalFillBlend(VideoStabilizerTemporalFill):
    """The Temporal Fill node with an exposure-matched, feathered seam (temporal_fill.py: `feather`, `exposure`).  Not one of
    the reference's nodes: it is listed by VideoStabilizerAmdFillBlendExtension and kept out of NODE_CLASSES."""

    @classmethod
    def define_schema(cls) -> io.Schema:
        schema = _schema("video_stabilizer_temporal_fill_blend", "Video Stabilizer Temporal Fill (Blended)",
                         description=("Video Stabilizer Temporal Fill whose filled pixels are matched to the frame's exposure and fade into "
                                      "the frame's own content over a feather, instead of meeting it at a hard cut."))
        base = VideoStabilizerTemporalFill.define_schema()
        schema.inputs = list(base.inputs) + [
            io.Int.Input("feather", default=16, min=0, max=64, display_name="Feather",
                         tooltip=("Width in source pixels over which the frame's own border fades into the neighbour's content; "
                                  "0 keeps the hard seam.")),
            io.Boolean.Input("match_exposure", default=True, display_name="Match Exposure",
                             tooltip="Scale what a neighbouring frame supplies to this frame's brightness, per channel."),
        ]
        schema.outputs = list(base.outputs)
        return schema

    @classmethod
    def execute(cls, frames: Any, frames_stabilized: Any, padding_mask: Any, meta: dict, radius: int, interpolation: str,
                feather: int, match_exposure: bool) -> io.NodeOutput:
        if isinstance(feather, bool):
            raise ValueError(f"feather={feather!r} is not an integer in 0..64")
        return cls._fill(frames, frames_stabilized, padding_mask, meta, radius, interpolation, feather=feather,
                         exposure=match_exposure)


class VideoStabilizerSharpnessTransfer(io.ComfyNode):
    """Repairs the shake-blurred frames of a Flow / Classic result from sharper neighbouring frames (sharpness_transfer.py),
    from the meta JSON alone, like the Temporal Fill node -- in front of which it belongs, since a filled pixel is no longer
    marked as padding.  Not one of the reference's nodes: it is listed by VideoStabilizerAmdSharpnessExtension and kept out
    of NODE_CLASSES."""

    @classmethod
    def define_schema(cls) -> io.Schema:
        schema = _schema("video_stabilizer_sharpness_transfer", "Video Stabilizer Sharpness Transfer",
                         description=("Pulls the pixels of frames a camera jolt blurred towards what sharper neighbouring frames show there, "
                                      "using the stabilizer's own motion metadata; frames with no sharper neighbour pass through unchanged."))
        schema.inputs = [
            io.Image.Input("frames", display_name="Frames", tooltip="The original (unstabilized) frames."),
            io.Image.Input("frames_stabilized", display_name="Stabilized Frames"),
            JSONType.Input("meta", display_name="Motion Meta"),
            io.Int.Input("radius", default=2, min=1, max=16, display_name="Radius",
                         tooltip="Frames before and after each frame that may lend it their sharpness."),
            io.Float.Input("alpha", default=16.0, min=0.0, max=1024.0, step=0.5, display_name="Alpha",
                           tooltip="How fast a neighbour's sample that disagrees with the pixel loses its weight; 0 averages."),
            io.Mask.Input("padding_mask", display_name="Padding Mask", optional=True,
                          tooltip="The stabilizer's padding mask; padded pixels are left alone.  Without it every pixel is own."),
        ]
        schema.outputs = [
            io.Image.Output("frames", display_name="Frames"),
            io.String.Output("meta", display_name="Meta"),
        ]
        return schema

    @classmethod
    def execute(cls, frames: Any, frames_stabilized: Any, meta: dict, radius: int, alpha: float, padding_mask: Any = None) -> io.NodeOutput:
        plan = temporal_fill.plan_from_meta(meta)   # ValueError naming the missing key, before any GPU work
        radius, alpha = sharpness_transfer.check_request(radius, alpha) or (0, 0.0)
        if radius == 0:
            raise ValueError("sharpness transfer: radius=0 transfers nothing; the node needs a radius in 1..16")
        context = hm._normalize_video_input(frames)
        out_context = hm._normalize_video_input(frames_stabilized)
        _check_clips_against_plan("sharpness transfer", plan, context, out_context)
        ctx = native.default_context()
        src = _device_frames(context, ctx)
        # the transfer works in place: on a copy, so the caller's tensor (another node's cached output) stays as it is
        dst = out_context.device_batch(ctx).clone()
        mask = None if padding_mask is None else _stabilizer_mask("sharpness transfer", padding_mask, dst, ctx)
        block = sharpness_transfer.transfer_on_device(ctx, src, dst, mask, plan["final_matrices"], plan["transitions"],
                                                      plan["confidences"], radius, alpha)
        return io.NodeOutput(_image_out(dst, out_context), json.dumps({"sharpness_transfer": block}))


def _variant_schema(cls, inputs: list, outputs: list) -> io.Schema:
    schema = _schema(*cls.NODE)
    schema.inputs, schema.outputs = inputs, outputs
    return schema


# the nine sockets of _estimator_inputs, which are _run_estimator_node's arguments behind the estimator
_ESTIMATOR_ARGS = ("frames", "frame_rate", "framing_mode", "transform_mode", "camera_lock", "strength", "smooth", "keep_fov",
                   "padding_color")


class _FlowVariant(io.ComfyNode):
    """An estimator node with the sockets of one `_stabilize_frames` feature.  A subclass states, next to its docstring:

    NODE       (node id, display name, description)
    ESTIMATOR  the estimator it runs
    BASE       the node whose inputs it starts from
    FIXED      {socket id: value}: base sockets it does not show, and what the pipeline gets in their place
    sockets()  its own sockets, fresh on every call; one with a base socket's id takes that socket's place, the others follow
    extras()   from the values of every socket behind the base nine (its parameters: their ids in the schema's order, with a
               default where a caller may leave one out) to the keyword extras of _stabilize_frames

    and gets its schema and an `execute` with the sockets as parameters, positional or by keyword, which hands on through the
    module's _run_estimator_node as it is at the time of the call."""

    ESTIMATOR = "flow"
    BASE = VideoStabilizerFlow
    FIXED: dict = {}

    @staticmethod
    def sockets() -> list:
        return []

    def __init_subclass__(cls, **kwargs) -> None:
        super().__init_subclass__(**kwargs)
        cls.FIXED = {**getattr(cls.BASE, "FIXED", {}), **cls.FIXED}
        positional = inspect.Parameter.POSITIONAL_OR_KEYWORD
        signature = inspect.Signature([inspect.Parameter(name, positional) for name in ("cls",) + _ESTIMATOR_ARGS if name not in cls.FIXED]
                                      + list(inspect.signature(cls.extras).parameters.values()))

        def execute(cls, *args, **kwargs) -> io.NodeOutput:
            given = signature.bind(cls, *args, **kwargs)
            given.apply_defaults()
            values = {**cls.FIXED, **given.arguments}
            del values["cls"]
            nine = [values.pop(name) for name in _ESTIMATOR_ARGS]
            return _run_estimator_node(cls.ESTIMATOR, *nine, **cls.extras(**values))

        execute.__signature__ = signature
        cls.execute = classmethod(execute)

    @classmethod
    def define_schema(cls) -> io.Schema:
        inputs = {s.id: s for s in cls.BASE.define_schema().inputs}   # in order: a replaced socket keeps its place
        inputs.update((s.id, s) for s in cls.sockets())
        return _variant_schema(cls, [s for s in inputs.values() if s.id not in cls.FIXED], _estimator_outputs())


def _two_model_transform_mode(tooltip: str, default: str = "similarity"):
    """`transform_mode` of a variant that cannot run a perspective fit."""
    return io.Combo.Input("transform_mode", options=["translation", "similarity"], default=default, display_name="Transform Mode",
                          tooltip=tooltip)


class VideoStabilizerFlowMasked(_FlowVariant):
    """The Flow node with an estimation mask: the pixels of `exclude_mask` (a segmentation of the moving subject, or one mask
    for a burnt-in logo) take no part in the camera-motion fit.  Not one of the reference's nodes: it is registered by the
    extension but kept out of NODE_CLASSES."""

    NODE = ("video_stabilizer_flow_masked", "Video Stabilizer Flow (Masked)",
            "Video Stabilizer Flow that estimates the camera motion from the pixels outside a mask, so that a "
            "moving subject in front of the camera does not become the motion that is removed.")

    @staticmethod
    def sockets() -> list:
        return [
            io.Mask.Input("exclude_mask", display_name="Exclude Mask",
                          tooltip=("Per-frame mask (or one mask for the whole clip) at the frames' resolution; values above "
                                   "0.5 mark pixels the motion estimate must not use.")),
            io.Int.Input("mask_margin", default=16, min=0, max=64, display_name="Mask Margin",
                         tooltip="Safety margin around the mask, in pixels of the estimation image (long side 960)."),
        ]

    @staticmethod
    def extras(exclude_mask, mask_margin) -> dict:
        return dict(estimation_mask=exclude_mask, mask_margin=int(mask_margin))


class VideoStabilizerFlowScenes(_FlowVariant):
    """The Flow node on an edited clip: hard cuts are found from the motion-compensated residual of every pair
    (scene_cuts.py) and every shot is stabilized on its own path, under one common framing.  Not one of the reference's
    nodes: it is listed by an extension but kept out of NODE_CLASSES."""

    NODE = ("video_stabilizer_flow_scenes", "Video Stabilizer Flow (Scene-Aware)",
            "Video Stabilizer Flow that detects hard cuts and stabilizes each shot separately, so that a cut "
            "neither enters the camera path nor pushes the frames on both sides of it out of place.")

    @staticmethod
    def sockets() -> list:
        return [
            io.Float.Input("cut_threshold", default=scene_cuts.DEFAULT_CUT_THRESHOLD, min=0.0, max=255.0, step=0.1, display_name="Cut Threshold",
                           tooltip=("Mean absolute difference (0..255) of two consecutive frames after motion compensation at "
                                    "and above which the pair is a cut.  0 uses the default, which was calibrated on "
                                    "synthetic clips only: lower it if cuts between similar scenes are missed.")),
        ]

    @staticmethod
    def extras(cut_threshold) -> dict:
        return dict(scene_cuts="auto", cut_threshold=float(cut_threshold) if cut_threshold else None)


class VideoStabilizerFlowMesh(_FlowVariant):
    """The Flow node with a mesh warp behind the global fit: the residual motion one matrix per frame cannot express
    (parallax, rolling-shutter skew, lens breathing) is measured per mesh vertex and smoothed like the global path
    (mesh_warp.py).  Not one of the reference's nodes: it is listed by an extension but kept out of NODE_CLASSES."""

    NODE = ("video_stabilizer_flow_mesh", "Video Stabilizer Flow (Mesh)",
            "Video Stabilizer Flow that also removes the slow local wobble a single global transform per frame "
            "leaves behind, with a coarse mesh of per-vertex corrections.")

    @staticmethod
    def sockets() -> list:
        return [
            io.Int.Input("mesh_cols", default=DEFAULT_CELLS[0], min=CELLS_MIN, max=CELLS_MAX, display_name="Mesh Columns",
                         tooltip="Cells of the mesh across the frame."),
            io.Int.Input("mesh_rows", default=DEFAULT_CELLS[1], min=CELLS_MIN, max=CELLS_MAX, display_name="Mesh Rows",
                         tooltip="Cells of the mesh down the frame."),
            io.Float.Input("max_shift", default=0.0, min=0.0, max=512.0, step=0.5, display_name="Max Shift",
                           tooltip=("Largest per-vertex correction in pixels, per axis.  0 uses the default, 1/64 of the frame's "
                                    "width, which has been tried on synthetic clips only: lower it if the picture warps.")),
        ]

    @staticmethod
    def extras(mesh_cols, mesh_rows, max_shift) -> dict:
        return dict(mesh_warp=(int(mesh_cols), int(mesh_rows)), mesh_max_shift=float(max_shift) if max_shift else None)


class VideoStabilizerFlowMeshMotion(_FlowVariant):
    """The Flow (Mesh) node that also records its per-vertex offsets in the meta (mesh_motion=True), so that Motion Apply
    (Mesh) can apply the same warp to a companion clip or undo it.  Not one of the reference's nodes: it is listed by an
    extension but kept out of NODE_CLASSES."""

    NODE = ("video_stabilizer_flow_mesh_motion", "Video Stabilizer Flow (Mesh Motion)",
            "Video Stabilizer Flow (Mesh) whose meta also carries the mesh's per-vertex offsets, which Video "
            "Stabilizer Motion Apply (Mesh) needs to repeat or undo the warp.")
    BASE = VideoStabilizerFlowMesh

    @staticmethod
    def extras(mesh_cols, mesh_rows, max_shift) -> dict:
        return dict(VideoStabilizerFlowMesh.extras(mesh_cols, mesh_rows, max_shift), mesh_motion=True)


class VideoStabilizerFlowZoom(_FlowVariant):
    """The Flow node with a dynamic zoom instead of padding: every frame is zoomed about the centre just enough to hide
    its own border, and the zoom is smoothed over a window so that it never pumps (dynamic_zoom.py).  Framing is fixed to
    crop_and_pad.  Not one of the reference's nodes: it is listed by an extension but kept out of NODE_CLASSES."""

    NODE = ("video_stabilizer_flow_zoom", "Video Stabilizer Flow (Dynamic Zoom)",
            "Video Stabilizer Flow whose borders are hidden by a per-frame zoom that follows the shake: calm "
            "stretches keep their field of view, only the shaky ones are zoomed in.")
    FIXED = {"framing_mode": "crop_and_pad"}

    @staticmethod
    def sockets() -> list:
        return [
            io.Float.Input("zoom_window", default=DEFAULT_WINDOW_S, min=0.05, max=WINDOW_MAX_S, step=0.05, display_name="Zoom Window",
                           tooltip=("Seconds over which the zoom is smoothed: it starts rising this long before a shake and "
                                    "settles this long after it.  The default has been tried on synthetic clips only.")),
            io.Float.Input("zoom_limit", default=DEFAULT_ZOOM_LIMIT, min=ZOOM_LIMIT_MIN, max=ZOOM_LIMIT_MAX, step=0.05,
                           display_name="Zoom Limit",
                           tooltip=("Largest zoom factor.  Frames that would need more keep some padding, which the padding "
                                    "mask and the meta report.  The default has been tried on synthetic clips only.")),
        ]

    @staticmethod
    def extras(zoom_window, zoom_limit) -> dict:
        return dict(dynamic_zoom=float(zoom_window), zoom_limit=float(zoom_limit))


class VideoStabilizerFlowSubject(_FlowVariant):
    """The Flow node locked on a subject: `subject_mask` (a per-frame segmentation of a person, face, product or vehicle) is
    reduced to the subject's centroid and area in every frame (subject_lock.py), and those -- not the camera's motion -- are
    what the trajectory steadies: with Camera Lock the subject stays where frame 0 shows it.  Not one of the reference's
    nodes: it is listed by an extension but kept out of NODE_CLASSES."""

    NODE = ("video_stabilizer_subject", "Video Stabilizer Flow (Subject Lock)",
            "Video Stabilizer Flow that stabilizes on a masked subject instead of the background: the subject is "
            "held still (Camera Lock) or followed smoothly, without the drift of integrated optical flow.")
    ESTIMATOR = "subject"

    @staticmethod
    def sockets() -> list:
        return [
            _two_model_transform_mode("translation follows the subject's centroid; similarity also its size (the square root "
                                      "of the mask's area ratio), without rotation.", default="translation"),
            io.Mask.Input("subject_mask", display_name="Subject Mask",
                          tooltip=("Per-frame mask of the subject at the frames' resolution; values above 0.5 are the subject. "
                                   "Frames without a subject are interpolated from their neighbours.")),
        ]

    @staticmethod
    def extras(subject_mask) -> dict:
        return dict(subject_mask=subject_mask)


class VideoStabilizerFlowRolling(_FlowVariant):
    """The Flow node with the rolling-shutter correction: the final warp samples every source row where a sensor read out
    row by row showed it, so the lean and wobble that remain once the shake is gone ("jello") are taken out with it
    (rolling_shutter.py).  Readout 0 estimates the sensor's readout time from the clip.  Not one of the reference's nodes: it
    is listed by an extension but kept out of NODE_CLASSES."""

    NODE = ("video_stabilizer_flow_rolling", "Video Stabilizer Flow (Rolling Shutter)",
            "Video Stabilizer Flow that also removes the skew and wobble of a rolling shutter: each row is "
            "corrected for the time at which the sensor read it.")

    @staticmethod
    def sockets() -> list:
        return [
            _two_model_transform_mode("Select the geometric model fitted to the optical flow.  The row correction is a closed "
                                      "form of an affine image velocity, so perspective is not offered."),
            io.Float.Input("readout", default=0.0, min=-1.0, max=1.0, step=0.01, display_name="Readout",
                           tooltip=("Readout time of the sensor as a fraction of the frame interval; negative for a sensor "
                                    "read from the bottom up.  0 estimates it from the clip, which needs a clip whose "
                                    "camera accelerates; the meta reports what was found.")),
        ]

    @staticmethod
    def extras(readout=0.0) -> dict:
        return dict(rolling_shutter="auto" if float(readout) == 0.0 else float(readout))


class VideoStabilizerFlowRollingRefit(_FlowVariant):
    """The Rolling Shutter node with the refit: the pair transitions are fitted a second time on flow samples corrected for
    the readout, so that the fit no longer takes part of the skew for rotation and scale (rolling_shutter.py).  Not one of the
    reference's nodes: it is listed by an extension but kept out of NODE_CLASSES."""

    NODE = ("video_stabilizer_flow_rolling_refit", "Video Stabilizer Flow (Rolling Shutter, Refit)",
            "Video Stabilizer Flow (Rolling Shutter) that also estimates the camera motion a second time on flow "
            "samples corrected for the sensor's readout.")
    BASE = VideoStabilizerFlowRolling

    @staticmethod
    def sockets() -> list:
        return [
            io.Boolean.Input("refit", default=True, display_name="Refit",
                             tooltip=("Fit the frame-to-frame motion again on flow samples corrected for the readout.  Off: "
                                      "the Rolling Shutter node.")),
        ]

    @staticmethod
    def extras(readout=0.0, refit=True) -> dict:
        return dict(VideoStabilizerFlowRolling.extras(readout), rolling_refit=bool(refit))


class VideoStabilizerFlowAnchored(_FlowVariant):
    """The Flow node with drift correction: every frame is registered directly against a keyframe, so the error of the
    consecutive-pair estimates no longer adds up along the clip and a locked picture stays put (drift_correction.py).  Not
    one of the reference's nodes: it is listed by an extension but kept out of NODE_CLASSES."""

    NODE = ("video_stabilizer_flow_anchored", "Video Stabilizer Flow (Drift-Free)",
            "Video Stabilizer Flow that registers every frame against a keyframe, so that the small error of "
            "each pair estimate does not accumulate into a creeping picture.")

    @staticmethod
    def sockets() -> list:
        return [
            _two_model_transform_mode("Select the geometric model fitted to the optical flow.  The keyframe alignment updates "
                                      "a shift, a zoom and a rotation, so perspective is not offered."),
            io.Int.Input("keyframe_spacing", default=32, min=2, max=4096, step=1, display_name="Keyframe Spacing",
                         tooltip=("Frames between two keyframes.  Every frame is aligned to the latest keyframe before it and "
                                  "every keyframe to the previous one; the meta reports how many frames were refined.")),
        ]

    @staticmethod
    def extras(keyframe_spacing=32) -> dict:
        return dict(drift_correction=int(keyframe_spacing))


class VideoStabilizerFlowAnchoredExposure(_FlowVariant):
    """The Drift-Free node for handheld footage: the keyframe alignment also estimates a gain and an offset per frame, so that
    auto-exposure does not defeat it, and leaves the pixels of an optional `exclude_mask` out (drift_correction.py).  Not one
    of the reference's nodes: it is listed by an extension but kept out of NODE_CLASSES."""

    NODE = ("video_stabilizer_flow_anchored_exposure", "Video Stabilizer Flow (Drift-Free, Exposure-Matched)",
            "Video Stabilizer Flow (Drift-Free) whose keyframe alignment follows the camera's auto-exposure and "
            "ignores a masked moving subject.")
    BASE = VideoStabilizerFlowAnchored

    @staticmethod
    def sockets() -> list:
        return [
            io.Boolean.Input("match_exposure", default=True, display_name="Match Exposure",
                             tooltip=("Estimate a brightness gain and offset of every frame against its keyframe next to the "
                                      "motion; the meta reports them.")),
            io.Mask.Input("exclude_mask", display_name="Exclude Mask", optional=True,
                          tooltip=("Per-frame mask (or one mask for the whole clip) at the frames' resolution; values above "
                                   "0.5 mark pixels neither the motion estimate nor the keyframe alignment may use.")),
            io.Int.Input("mask_margin", default=16, min=0, max=64, display_name="Mask Margin",
                         tooltip="Safety margin around the mask, in pixels of the estimation image (long side 960)."),
        ]

    @staticmethod
    def extras(keyframe_spacing=32, match_exposure=True, exclude_mask=None, mask_margin=16) -> dict:
        masked = {} if exclude_mask is None else dict(estimation_mask=exclude_mask, mask_margin=int(mask_margin), drift_mask=True)
        return dict(VideoStabilizerFlowAnchored.extras(keyframe_spacing), drift_exposure=True if match_exposure else None, **masked)


class VideoStabilizerFlowLevel(_FlowVariant):
    """The Flow node that also levels the picture: the roll of every frame is measured from the orientation of its edges,
    one offset per shot -- or one that varies slowly -- is taken from it, and every frame is turned upright about the centre
    (horizon_level.py).  Framing is fixed to crop_and_pad.  Not one of the reference's nodes: it is listed by an extension but
    kept out of NODE_CLASSES."""

    NODE = ("video_stabilizer_flow_level", "Video Stabilizer Flow (Horizon Level)",
            "Video Stabilizer Flow that also levels the horizon: a clip shot a few degrees off level comes out "
            "steady and upright.")
    FIXED = {"framing_mode": "crop_and_pad"}

    @staticmethod
    def sockets() -> list:
        return [
            _two_model_transform_mode("Select the geometric model fitted to the optical flow.  A homography has no single roll, "
                                      "so perspective is not offered."),
            io.Float.Input("level_window", default=0.0, min=0.0, max=LEVEL_WINDOW_MAX_S, step=0.05, display_name="Level Window",
                           tooltip=("Seconds over which the roll offset may vary, for a camera that slowly tips over.  0 takes "
                                    "one offset for every shot.")),
            io.Float.Input("level_limit", default=DEFAULT_LIMIT_DEG, min=0.5, max=LIMIT_MAX_DEG - 0.5, step=0.5,
                           display_name="Level Limit",
                           tooltip=("Largest correction in degrees.  Edges give the roll modulo 90 degrees only, so it stays "
                                    "below 45.  The default has been tried on synthetic clips only.")),
        ]

    @staticmethod
    def extras(level_window=0.0, level_limit=DEFAULT_LIMIT_DEG) -> dict:
        return dict(horizon_level=True if float(level_window) == 0.0 else float(level_window), horizon_limit=float(level_limit))


class _ApplyVariant(io.ComfyNode):
    """Motion Apply for a run whose warp is more than one matrix per frame.  A subclass states NODE as a Flow variant does and
    REPLAY, the keyword of apply_motion that selects its replay.  Bilinear, no motion blur."""

    REPLAY: dict = {}

    @classmethod
    def define_schema(cls) -> io.Schema:
        return _variant_schema(cls, [
            io.Image.Input("frames", display_name="Frames"),
            JSONType.Input("meta", display_name="Meta"),
            io.Combo.Input("framing_mode", options=["crop_and_pad", "expand"], default="crop_and_pad",
                           display_name="Framing Mode"),
            io.Color.Input("padding_color", default="#7F7F7F", display_name="Padding Color",
                           tooltip="HEX padding color used where warping exposes empty pixels."),
        ], _clip_outputs())

    @classmethod
    def execute(cls, frames: Any, meta: dict, framing_mode: str, padding_color: str) -> io.NodeOutput:
        context = hm._normalize_video_input(frames)
        result = apply_motion(context, meta, hm._parse_padding_color(padding_color), framing_mode=framing_mode,
                              interpolation="bilinear", keep_on_device=True, **cls.REPLAY)
        return io.NodeOutput(_image_out(result.frames, context), _mask_out(result.masks), result.meta)


class VideoStabilizerMotionApplyMesh(_ApplyVariant):
    """Motion Apply for a mesh-warped run (apply_motion's mesh=True): on the run's source frames (or a companion clip of
    their size) it applies the recorded matrices and mesh again, on its stabilized frames it restores the original camera
    motion through the mesh warp's per-pixel inverse.  Bilinear, no motion blur.  Not one of the reference's nodes."""

    NODE = ("video_stabilizer_motion_apply_mesh", "Video Stabilizer Motion Apply (Mesh)",
            "Applies or undoes the motion of a Video Stabilizer Flow (Mesh Motion) run, per-vertex mesh "
            "corrections included, and emits a padding mask.")
    REPLAY = {"mesh": True}


class VideoStabilizerMotionApplyRolling(_ApplyVariant):
    """Motion Apply for a rolling-shutter run (apply_motion's rolling=True): on the run's source frames (or a companion clip
    of their size) it applies the recorded matrices and row correction again, on its stabilized frames it restores the
    original camera motion and skew through the rolling warp's closed-form inverse.  Bilinear, no motion blur.  Not one of the
    reference's nodes: it is listed by an extension but kept out of NODE_CLASSES."""

    NODE = ("video_stabilizer_motion_apply_rolling", "Video Stabilizer Motion Apply (Rolling Shutter)",
            "Applies or undoes the motion of a Video Stabilizer Flow (Rolling Shutter) run, per-row readout "
            "correction included, and emits a padding mask.")
    REPLAY = {"rolling": True}


class VideoStabilizerPaddingFill(io.ComfyNode):
    """Fills the padded pixels of any frames / padding mask pair from each frame's own valid pixels by pyramid push-pull
    (spatial_fill.py): the outputs of any node of this package, or of the unchanged reference nodes.  The mask is not an
    output: it stays what it was, for a downstream in-painter.  Not one of the reference's nodes: it is listed by an
    extension but kept out of NODE_CLASSES."""

    @classmethod
    def define_schema(cls) -> io.Schema:
        schema = _schema("video_stabilizer_padding_fill", "Video Stabilizer Padding Fill",
                         description=("Fills the padding a stabilizer left with a smooth continuation of each frame's own content "
                                      "(push-pull), a far better start for an in-painter than a flat colour; the padding mask still "
                                      "marks the invented pixels."))
        schema.inputs = [
            io.Image.Input("frames", display_name="Frames", tooltip="Stabilized frames with padding."),
            io.Mask.Input("padding_mask", display_name="Padding Mask", tooltip="[N,H,W], or [1,H,W] for every frame."),
        ]
        schema.outputs = [
            io.Image.Output("frames", display_name="Frames"),
            io.String.Output("meta", display_name="Meta"),
        ]
        return schema

    @classmethod
    def execute(cls, frames: Any, padding_mask: Any) -> io.NodeOutput:
        context = hm._normalize_video_input(frames)
        dims, lead = _check_clip_and_mask("padding fill", context, padding_mask, optional=False)
        ctx = native.default_context()
        # the fill works in place: on a copy, so the caller's tensor (another node's cached output) stays as it is
        dst = _device_frames(context, ctx).clone()
        mask = _place_socket_mask(padding_mask, lead, dims, ctx)
        block = spatial_fill.fill_on_device(ctx, dst, mask)
        return io.NodeOutput(_image_out(dst, context), json.dumps({"spatial_fill": block}))


class VideoStabilizerStabilityReport(io.ComfyNode):
    """How steady a clip is, as a number: the inter-frame transformation fidelity (stability.py) of any frames, under their
    padding mask if one is given, and next to the unstabilized clip's if that is given.  Reads its inputs and returns the
    block as JSON.  Not one of the reference's nodes: it is listed by an extension but kept out of NODE_CLASSES."""

    @classmethod
    def define_schema(cls) -> io.Schema:
        schema = _schema("video_stabilizer_stability_report", "Video Stabilizer Stability Report",
                         description=("Mean PSNR between consecutive frames (ITF) over the pixels both frames really show; with the "
                                      "unstabilized clip connected, also its ITF and the gain in dB."))
        schema.inputs = [
            io.Image.Input("frames", display_name="Frames", tooltip="The clip to measure, e.g. stabilized frames."),
            io.Mask.Input("padding_mask", display_name="Padding Mask", optional=True,
                          tooltip="[N,H,W], or [1,H,W] for every frame; padded pixels stay out of the measure."),
            io.Image.Input("reference_frames", display_name="Reference Frames", optional=True,
                           tooltip="The unstabilized clip, for `before` and `gain_db`."),
        ]
        schema.outputs = [io.String.Output("meta", display_name="Meta")]
        return schema

    @classmethod
    def execute(cls, frames: Any, padding_mask: Any = None, reference_frames: Any = None) -> io.NodeOutput:
        context = hm._normalize_video_input(frames)
        dims, lead = _check_clip_and_mask("stability report", context, padding_mask)
        reference = None if reference_frames is None else hm._normalize_video_input(reference_frames)
        if reference is not None and len(reference.frames) == 0:
            raise ValueError("stability report: socket 'reference_frames' holds no frame")
        ctx = native.default_context()
        mask = _place_socket_mask(padding_mask, lead, dims, ctx)
        after = stability.itf(_device_frames(context, ctx), mask, ctx=ctx)
        before = None if reference is None else stability.itf(_device_frames(reference, ctx), None, ctx=ctx)
        return io.NodeOutput(json.dumps({"stability": stability.report_block(before, after)}))


NODE_CLASSES = [VideoStabilizerClassic, VideoStabilizerFlow, VideoStabilizerMotionApply, VideoStabilizerShakeGenerator,
                VideoStabilizerShakeGeneratorManual, VideoStabilizerInverse]


class VideoStabilizerMaskGrow(io.ComfyNode):
    """ComfyUI's GrowMask on the GPU, with an outward feather and a temporal hold (mask_handoff.py): the node between a
    stabilizer's padding mask and an outpainter.  `mask`, `expand` and `tapered_corners` carry GrowMask's socket names and
    defaults, so it takes GrowMask's place in the reference's two workflows.  Not one of the reference's nodes: it is listed
    by an extension but kept out of NODE_CLASSES."""

    @classmethod
    def define_schema(cls) -> io.Schema:
        schema = _schema("video_stabilizer_mask_grow", "Video Stabilizer Mask Grow",
                         description=("Grows (or shrinks) a padding mask as GrowMask does, on the GPU, optionally holds it over neighbouring "
                                      "frames so the repaint region stands still, and feathers its edge outwards."))
        schema.inputs = [
            io.Mask.Input("mask", display_name="Mask", tooltip="[N,H,W] or [H,W]."),
            io.Int.Input("expand", default=5, min=-64, max=64, step=1, display_name="Expand",
                         tooltip="Pixels of growth; negative shrinks."),
            io.Boolean.Input("tapered_corners", default=True, display_name="Tapered Corners",
                             tooltip="True grows over a diamond (GrowMask's cross footprint), False over a square."),
            io.Int.Input("feather", default=0, min=0, max=64, step=1, display_name="Feather",
                         tooltip="Pixels of linear ramp added outside the grown mask."),
            io.Int.Input("hold", default=0, min=0, max=16, step=1, display_name="Hold",
                         tooltip="Frames before and after over which the mask is held (maximum), before it is grown."),
        ]
        schema.outputs = [io.Mask.Output("mask", display_name="Mask")]
        return schema

    @classmethod
    def execute(cls, mask: Any, expand: int = 5, tapered_corners: bool = True, feather: int = 0, hold: int = 0) -> io.NodeOutput:
        # every check comes before any GPU work
        request = mask_handoff.check_request(expand, feather, hold, tapered_corners)
        if not (hasattr(mask, "dtype") and hasattr(mask, "shape")):
            raise ValueError(f"mask grow: socket 'mask' must be a floating-point MASK tensor, got {type(mask).__name__}")
        if "float" not in str(mask.dtype):
            raise ValueError(f"mask grow: socket 'mask' must be a floating-point MASK, got {mask.dtype}")
        shape = tuple(int(v) for v in mask.shape)
        if len(shape) not in (2, 3) or min(shape) < 1:
            raise ValueError(f"mask grow: socket 'mask' of shape {tuple(mask.shape)} is not [N,H,W] or [H,W]")
        ctx = native.default_context()
        torch = ctx.torch
        m = mask if isinstance(mask, torch.Tensor) else torch.from_numpy(np.asarray(mask))
        m = m.to(device=ctx.device, dtype=torch.float32).reshape(shape[-3:] if len(shape) == 3 else (1,) + shape).contiguous()
        out, _ = mask_handoff.handoff_on_device(ctx, m, request)
        out = out.reshape(shape)
        # a feathered mask is neither 0 / 1 nor a motion-blur level: levels = 1 lets a 0 / 1 result cross as bytes, and the
        # download itself takes the float path for a mask with any other value -- the bits arrive either way
        return io.NodeOutput(_mask_out(out, 1))


class VideoStabilizerDeflicker(io.ComfyNode):
    """Takes the exposure steps between consecutive frames out of a stabilized clip (deflicker.py): measured on the ORIGINAL
    frames through the stabilizer's own transitions, from the meta JSON alone, like the Temporal Fill node -- in front of which
    it belongs, since a filled pixel is no longer marked as padding.  Without a meta the camera is taken to be locked off (a
    tripod shot, a timelapse): identity transitions, and `frames_stabilized` may be `frames` itself.  Not one of the
    reference's nodes: it is listed by VideoStabilizerAmdDeflickerExtension and kept out of NODE_CLASSES."""

    @classmethod
    def define_schema(cls) -> io.Schema:
        schema = _schema("video_stabilizer_deflicker", "Video Stabilizer Deflicker",
                         description=("Measures the exposure change between consecutive frames on registered pixels, robustly against moving "
                                      "subjects, and multiplies every frame by the high-pass of that chain; a deliberate exposure ramp stays."))
        schema.inputs = [
            io.Image.Input("frames", display_name="Frames", tooltip="The original (unstabilized) frames."),
            io.Image.Input("frames_stabilized", display_name="Stabilized Frames",
                           tooltip="The frames to correct; without a meta they may be the original frames themselves."),
            io.Mask.Input("padding_mask", display_name="Padding Mask", optional=True,
                          tooltip="The stabilizer's padding mask; padded pixels keep their colour.  Without it every pixel is own."),
            JSONType.Input("meta", display_name="Motion Meta", optional=True,
                           tooltip="A Flow / Classic stabilizer's meta.  Without it the camera is taken to be locked off."),
            io.Float.Input("window", default=1.0, min=0.05, max=60.0, step=0.05, display_name="Window (s)",
                           tooltip="The exposure chain is smoothed over this many seconds; what is faster is taken out."),
            io.Combo.Input("mode", options=["exposure", "rgb"], default="exposure", display_name="Mode",
                           tooltip="exposure: one gain for the three colours.  rgb: one per colour, which also steadies white balance."),
        ]
        schema.outputs = [
            io.Image.Output("frames", display_name="Frames"),
            io.String.Output("meta", display_name="Meta"),
        ]
        return schema

    @classmethod
    def execute(cls, frames: Any, frames_stabilized: Any, padding_mask: Any = None, meta: Any = None, window: float = 1.0,
                mode: str = "exposure") -> io.NodeOutput:
        # every check comes before any GPU work
        request = deflicker.check_request(window, mode)
        if request is None:
            raise ValueError(f"deflicker: window={window!r} switches the node off; it needs a window in seconds in (0, 60]")
        context = hm._normalize_video_input(frames)
        out_context = context if frames_stabilized is frames else hm._normalize_video_input(frames_stabilized)
        n = len(context.frames)
        if n < 2 or len(out_context.frames) != n:
            raise ValueError(f"deflicker: needs at least two frames and as many stabilized as original ones, got {n} original and "
                             f"{len(out_context.frames)} stabilized frames")
        segments = None
        if meta is not None:
            plan = temporal_fill.plan_from_meta(meta)   # ValueError naming the missing key
            if len(plan["final_matrices"]) != n:
                raise ValueError(f"deflicker: meta describes {len(plan['final_matrices'])} frames, got {n}")
            _check_clips_against_plan("deflicker", plan, context, out_context)   # (the sizes: both clips have the plan's n frames)
            transitions, confidences = plan["transitions"], plan["confidences"]
            fps = meta.get("fps_effective")
            if isinstance(meta.get("scene_cuts"), dict) and meta["scene_cuts"].get("cuts"):
                segments = scene_cuts.segments_from_cuts(meta["scene_cuts"]["cuts"], n)
        else:
            transitions, confidences, fps = np.tile(np.eye(3, dtype=np.float32), (n - 1, 1, 1)), np.ones(n - 1), None
        fps_effective = _fps_fields(context, fps)[0]
        ctx = native.default_context()
        src = _device_frames(context, ctx)
        # the correction works in place: on a copy, so the caller's tensor (another node's cached output) stays as it is
        dst = (src if out_context is context else _device_frames(out_context, ctx)).clone()
        mask = None if padding_mask is None else _stabilizer_mask("deflicker", padding_mask, dst, ctx)
        block = deflicker.deflicker_on_device(ctx, request, src, dst, mask, transitions, confidences, fps_effective, segments)
        return io.NodeOutput(_image_out(dst, out_context), json.dumps({"deflicker": block}))


class VideoStabilizerCleanPlate(io.ComfyNode):
    """The clean plate of a REGISTERED clip (clean_plate.py) -- a tripod shot, or the output of a stabilizer run with camera
    lock at strength 1 -- taken as one shot: the per-pixel median over time of what the frames show under their padding mask,
    the frames with their leftover padding filled from it, and the matte of what differs from it.  Not one of the reference's
    nodes: it is listed by VideoStabilizerAmdPlateExtension and kept out of NODE_CLASSES."""

    @classmethod
    def define_schema(cls) -> io.Schema:
        schema = _schema("video_stabilizer_clean_plate", "Video Stabilizer Clean Plate",
                         description=("The background of a locked shot with everything that moves taken out (the per-pixel median over time), "
                                      "the frames with their padding filled from it, and the difference matte."))
        schema.inputs = [
            io.Image.Input("frames", display_name="Frames", tooltip="A registered clip: a tripod shot or a camera-locked stabilizer output."),
            io.Mask.Input("padding_mask", display_name="Padding Mask", optional=True,
                          tooltip="[N,H,W], or [1,H,W] for every frame; padded pixels do not vote.  Without it every pixel is own."),
            io.Boolean.Input("fill", default=True, display_name="Fill", tooltip="Fill the padded pixels from the plate and clear their mask."),
            io.Int.Input("min_count", default=1, min=1, max=clean_plate.SAMPLES_MAX, step=1, display_name="Min Count",
                         tooltip="Frames that must have seen a plate pixel before it fills anything."),
            io.Float.Input("matte_threshold", default=clean_plate.DEFAULT_MATTE_THRESHOLD, min=0.0, max=1.0, step=0.01, display_name="Matte Threshold",
                           tooltip="A pixel is matte where some channel differs from the plate by more than this.  A choice, not a calibration."),
            io.Int.Input("matte_min_count", default=clean_plate.DEFAULT_MATTE_MIN_COUNT, min=1, max=clean_plate.SAMPLES_MAX, step=1, display_name="Matte Min Count",
                         tooltip="Frames that must have seen a plate pixel before it can mark a matte.  A choice, not a calibration."),
        ]
        schema.outputs = [
            io.Image.Output("plate", display_name="Plate"),
            io.Image.Output("frames", display_name="Frames"),
            io.Mask.Output("padding_mask", display_name="Padding Mask"),
            io.Mask.Output("matte", display_name="Matte"),
            io.String.Output("meta", display_name="Meta"),
        ]
        return schema

    @classmethod
    def execute(cls, frames: Any, padding_mask: Any = None, fill: bool = True, min_count: int = 1, matte_threshold: float = 0.1,
                matte_min_count: int = 3) -> io.NodeOutput:
        # every check comes before any GPU work
        if not isinstance(fill, (bool, np.bool_)):
            raise ValueError(f"clean plate: fill={fill!r} is not a bool")
        for name, value in (("min_count", min_count), ("matte_min_count", matte_min_count)):
            if isinstance(value, (bool, np.bool_)) or not isinstance(value, (int, np.integer)) or not 1 <= int(value) <= clean_plate.SAMPLES_MAX:
                raise ValueError(f"clean plate: {name}={value!r} is not an integer in 1..{clean_plate.SAMPLES_MAX}")
        if isinstance(matte_threshold, bool) or not isinstance(matte_threshold, (int, float)) or not 0.0 <= matte_threshold <= 1.0:
            raise ValueError(f"clean plate: matte_threshold={matte_threshold!r} is not a number in [0, 1]")
        context = hm._normalize_video_input(frames)
        dims, lead = _check_clip_and_mask("clean plate", context, padding_mask)
        ctx = native.default_context()
        src = _device_frames(context, ctx)
        # (a copy: the fill works in place, and the caller's tensor -- another node's cached output -- stays as it is)
        mask = _place_socket_mask(padding_mask, lead, dims, ctx, copy=True)
        plate, count, table = clean_plate.plate_on_device(ctx, src, mask)
        matte, matte_count = clean_plate.matte_on_device(ctx, src, mask, plate, count, None, float(matte_threshold), int(matte_min_count))
        block = {"version": 1, "samples": int((table >= 0).sum()), "matte_threshold": float(matte_threshold),
                 "matte_min_count": int(matte_min_count)}
        pixels = np.float32(dims[1] * dims[2])
        share = (matte_count.cpu().numpy().astype(np.float32) / pixels).astype(np.float64)
        block.update({"matte_fraction_mean": float(np.mean(share)), "matte_fraction_max": float(np.max(share))})
        dst = src
        if fill and mask is not None:
            dst = src.clone()
            block["plate_fill"] = clean_plate.fill_and_report(ctx, dst, mask, plate, count, table, None, int(min_count))
        if mask is None:
            mask = ctx.torch.zeros(dims, dtype=ctx.torch.float32, device=ctx.device)
        return io.NodeOutput(_image_out(plate, context), _image_out(dst, context), _mask_out(mask, 1), _mask_out(matte, 1),
                             json.dumps({"clean_plate": block}))


class VideoStabilizerAmdExtension(ComfyExtension):
    async def get_node_list(self) -> list:
        return list(NODE_CLASSES) + [VideoStabilizerTemporalFill]   # the six reference nodes + the temporal fill

    async def on_load(self) -> None:
        """Graph migration Inverse -> Motion Apply, as nodes/node_replacements.py:8-27 registers it (only inside
        a ComfyUI that exposes the node-replacement API)."""
        try:
            from comfy_api.latest import ComfyAPI  # type: ignore
        except ImportError:
            return
        api = ComfyAPI()
        await api.node_replacement.register(
            io.NodeReplace(
                new_node_id="video_stabilizer_motion_apply",
                old_node_id="video_stabilizer_inverse",
                old_widget_ids=["padding_color"],
                input_mapping=[
                    {"new_id": "frames", "old_id": "frames"},
                    {"new_id": "motion_meta", "old_id": "meta"},
                    {"new_id": "padding_color", "old_id": "padding_color"},
                    {"new_id": "framing_mode", "set_value": "crop_and_pad"},
                    {"new_id": "interpolation", "set_value": "bilinear"},
                ],
                output_mapping=[{"new_idx": 0, "old_idx": 0}, {"new_idx": 1, "old_idx": 1}, {"new_idx": 2, "old_idx": 2}],
            )
        )


def _extend(base: type, *added_nodes: type, name: str, doc: str) -> type:
    """A subclass of the extension `base` whose node list is base's plus `added_nodes`.  Every feature gets a class of its
    own, so that the extensions before it keep the lists they had and code that instantiates one sees what it saw."""

    async def get_node_list(self) -> list:
        return await base.get_node_list(self) + list(added_nodes)

    return type(name, (base,), {"__doc__": doc, "__module__": __name__, "get_node_list": get_node_list})


# One extension class per feature, each made from the one before it: (class name, added nodes, docstring), oldest first.  A new
# feature adds a row at the end; comfy_entrypoint() keeps returning the first.
_EXTENSION_CHAIN = [
    ("VideoStabilizerAmdMaskedExtension", [VideoStabilizerFlowMasked],
     "What comfy_entrypoint() hands to ComfyUI: the base extension's seven nodes plus Video Stabilizer Flow (Masked)."),
    ("VideoStabilizerAmdScenesExtension", [VideoStabilizerFlowScenes],
     "The masked extension's eight nodes plus Video Stabilizer Flow (Scene-Aware)."),
    ("VideoStabilizerAmdMeshExtension", [VideoStabilizerFlowMesh],
     "The scene-aware extension's nine nodes plus Video Stabilizer Flow (Mesh)."),
    ("VideoStabilizerAmdMeshApplyExtension", [VideoStabilizerFlowMeshMotion, VideoStabilizerMotionApplyMesh],
     "The mesh extension's ten nodes plus the two of the mesh round trip: Flow (Mesh Motion) and Motion Apply (Mesh)."),
    ("VideoStabilizerAmdFillExtension", [VideoStabilizerPaddingFill],
     "The mesh round trip extension's twelve nodes plus Video Stabilizer Padding Fill."),
    ("VideoStabilizerAmdReportExtension", [VideoStabilizerStabilityReport],
     "The fill extension's thirteen nodes plus Video Stabilizer Stability Report."),
    ("VideoStabilizerAmdZoomExtension", [VideoStabilizerFlowZoom],
     "The report extension's fourteen nodes plus Video Stabilizer Flow (Dynamic Zoom)."),
    ("VideoStabilizerAmdSubjectExtension", [VideoStabilizerFlowSubject],
     "The zoom extension's fifteen nodes plus Video Stabilizer Flow (Subject Lock)."),
    ("VideoStabilizerAmdFillBlendExtension", [VideoStabilizerTemporalFillBlend],
     "The subject extension's sixteen nodes plus Video Stabilizer Temporal Fill (Blended)."),
    ("VideoStabilizerAmdSharpnessExtension", [VideoStabilizerSharpnessTransfer],
     "The blended-fill extension's seventeen nodes plus Video Stabilizer Sharpness Transfer."),
    ("VideoStabilizerAmdHandoffExtension", [VideoStabilizerMaskGrow],
     "The sharpness extension's eighteen nodes plus Video Stabilizer Mask Grow."),
    ("VideoStabilizerAmdRollingExtension", [VideoStabilizerFlowRolling],
     "The hand-off extension's nineteen nodes plus Video Stabilizer Flow (Rolling Shutter)."),
    ("VideoStabilizerAmdRollingApplyExtension", [VideoStabilizerMotionApplyRolling],
     "The rolling-shutter extension's twenty nodes plus Video Stabilizer Motion Apply (Rolling Shutter)."),
    ("VideoStabilizerAmdAnchorExtension", [VideoStabilizerFlowAnchored],
     "The rolling round trip extension's twenty-one nodes plus Video Stabilizer Flow (Drift-Free)."),
    ("VideoStabilizerAmdAnchorExposureExtension", [VideoStabilizerFlowAnchoredExposure],
     "The drift-free extension's twenty-two nodes plus Video Stabilizer Flow (Drift-Free, Exposure-Matched)."),
    ("VideoStabilizerAmdRollingRefitExtension", [VideoStabilizerFlowRollingRefit],
     "The exposure-matched extension's twenty-three nodes plus Video Stabilizer Flow (Rolling Shutter, Refit)."),
    ("VideoStabilizerAmdDeflickerExtension", [VideoStabilizerDeflicker],
     "The refit extension's twenty-four nodes plus Video Stabilizer Deflicker."),
    ("VideoStabilizerAmdLevelExtension", [VideoStabilizerFlowLevel],
     "The deflicker extension's twenty-five nodes plus Video Stabilizer Flow (Horizon Level)."),
    ("VideoStabilizerAmdPlateExtension", [VideoStabilizerCleanPlate],
     "The level extension's twenty-six nodes plus Video Stabilizer Clean Plate."),
]

_latest = VideoStabilizerAmdExtension
for _name, _added, _doc in _EXTENSION_CHAIN:
    _latest = globals()[_name] = _extend(_latest, *_added, name=_name, doc=_doc)
del _latest, _name, _added, _doc
