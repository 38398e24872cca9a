"""The node layer's surface, pinned on the CPU: every node's schema, the registration, what each estimator / apply node hands
to the pipeline, and every refusal a post-warp node makes before it asks for the GPU context.

The fixture tests/golden/node_surface.json is written by

    python tests/test_node_surface_cpu.py --write

from the tree it runs in, and is compared item by item as serialised JSON, so that 16, 16.0 and True are three different
values.  It was written before nodes.py was restated (one Flow-variant table, one frame and mask intake, one extension
chain) and has not been edited since: a change of nodes.py that alters it alters what ComfyUI or a caller sees.

What the compat layer's stand-in sockets expose is all there is to pin: kind, direction, id and the options dictionary
(defaults, ranges, steps, tooltips, `optional`, display mode, display name), in order.
"""

from __future__ import annotations

import asyncio
import inspect
import json
import sys
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest

GOLDEN = Path(__file__).resolve().parent / "golden" / "node_surface.json"

N_NODES, N_EXTENSIONS = 27, 20
N_REFUSALS = 116   # the cases of _refusal_cases(), the 17 "valid" ones that reach the context included
REFUSING_NODES = ("TemporalFill", "TemporalFillBlend", "SharpnessTransfer", "PaddingFill", "StabilityReport", "MaskGrow",
                  "Deflicker", "CleanPlate")
ESTIMATOR_NODES = ("Flow", "Classic", "FlowMasked", "FlowScenes", "FlowMesh", "FlowMeshMotion", "FlowZoom", "FlowSubject",
                   "FlowRolling", "FlowRollingRefit", "FlowAnchored", "FlowAnchoredExposure", "FlowLevel")
APPLY_NODES = ("MotionApplyMesh", "MotionApplyRolling")


def _load():
    import __graft_entry__ as graft

    graft.load_package()
    import vstab_amd
    from vstab_amd import nodes

    return vstab_amd, nodes


def _text(value) -> str:
    """One item as it is compared: JSON with sorted keys (a tuple is a list; 16, 16.0 and true differ)."""
    return json.dumps(value, sort_keys=True, default=repr)


def _all_nodes(nodes) -> list:
    return asyncio.run(nodes.VideoStabilizerAmdPlateExtension().get_node_list())


# ---------------------------------------------------------------- 1. schemas

def _socket(s) -> dict:
    return {"kind": s.kind, "direction": s.direction, "id": s.id, "options": dict(s.options)}


def _signature(fn) -> list:
    return [[p.name, str(p.kind), None if p.default is inspect.Parameter.empty else {"default": p.default}]
            for p in inspect.signature(fn).parameters.values()]


def dump_schemas(nodes) -> dict:
    out = {}
    for cls in _all_nodes(nodes):
        s = cls.define_schema()
        out[cls.__name__] = {
            "module": cls.__module__, "doc": cls.__doc__, "execute": _signature(cls.execute),
            "node_id": s.node_id, "display_name": s.display_name, "category": s.category, "description": s.description,
            "extra": dict(s.extra), "inputs": [_socket(i) for i in s.inputs], "outputs": [_socket(o) for o in s.outputs],
        }
    return out


# ---------------------------------------------------------------- 2. registration

def dump_registration(vstab_amd, nodes) -> dict:
    from vstab_amd.comfy_compat import ComfyExtension

    extensions = {}   # the base extension and the nineteen made from it, in the module's order
    for name, value in vars(nodes).items():
        if isinstance(value, type) and issubclass(value, ComfyExtension) and value is not ComfyExtension:
            extensions[name] = {"name": value.__name__, "module": value.__module__, "doc": value.__doc__,
                                "bases": [b.__name__ for b in value.__bases__],
                                "nodes": [c.__name__ for c in asyncio.run(value().get_node_list())]}
    return {"NODE_CLASSES": [c.__name__ for c in nodes.NODE_CLASSES],
            "extensions": extensions,
            "entrypoint": type(asyncio.run(vstab_amd.comfy_entrypoint())).__name__}


# ---------------------------------------------------------------- 3. what each node hands on

def _schema_defaults(cls) -> dict:
    """Socket id -> the value a graph with untouched widgets sends: the schema default; a name for an image or a mask."""
    values = {}
    for s in cls.define_schema().inputs:
        if "default" in s.options:
            values[s.id] = s.options["default"]
        elif s.options.get("optional"):
            values[s.id] = None
        else:
            values[s.id] = s.kind.upper() + ":" + s.id
    return values


# both sides of every conversion an estimator node makes, and the values whose type it fixes (int(...) / float(...) / bool(...))
HANDOFF_VARIATIONS = {
    "FlowMasked": [{"mask_margin": 24.0}],
    "FlowScenes": [{"cut_threshold": 0}, {"cut_threshold": 0.0}, {"cut_threshold": 7.5}, {"cut_threshold": 7}],
    "FlowMesh": [{"max_shift": 0}, {"max_shift": 0.0}, {"max_shift": 3.5}, {"max_shift": 3}, {"mesh_cols": 12.0, "mesh_rows": 7.0}],
    "FlowMeshMotion": [{"max_shift": 0}, {"max_shift": 0.0}, {"max_shift": 3.5}, {"max_shift": 3}, {"mesh_cols": 12.0, "mesh_rows": 7.0}],
    "FlowZoom": [{"zoom_window": 2, "zoom_limit": 2}, {"zoom_window": 0.75, "zoom_limit": 1.5}],
    "FlowSubject": [{"transform_mode": "similarity", "camera_lock": True}],
    "FlowRolling": [{"readout": 0}, {"readout": 0.0}, {"readout": -0.25}, {"readout": 1}],
    "FlowRollingRefit": [{"readout": 0}, {"readout": -0.25}, {"refit": False}, {"refit": True}, {"refit": 0}, {"refit": 1},
                         {"readout": 0.5, "refit": False}],
    "FlowAnchored": [{"keyframe_spacing": 8}, {"keyframe_spacing": 8.0}],
    "FlowAnchoredExposure": [{"match_exposure": False}, {"match_exposure": True}, {"match_exposure": 0},
                             {"exclude_mask": "MASK:exclude_mask"}, {"exclude_mask": "MASK:exclude_mask", "mask_margin": 8.0},
                             {"exclude_mask": "MASK:exclude_mask", "match_exposure": False, "keyframe_spacing": 4.0},
                             {"mask_margin": 8}],
    "FlowLevel": [{"level_window": 0}, {"level_window": 0.0}, {"level_window": 2.5}, {"level_window": 2}, {"level_limit": 12},
                  {"level_limit": 12.5}],
}


def _handoff_calls(nodes) -> list:
    """[(node, case, args, kwargs)]: the schema defaults positionally and by keyword, every parameter that `execute` lets a caller
    leave out left out (one at a time and all together), and HANDOFF_VARIATIONS by keyword."""
    calls = []
    for short in ESTIMATOR_NODES + APPLY_NODES:
        cls = getattr(nodes, "VideoStabilizer" + short)
        values = _schema_defaults(cls)
        if short in APPLY_NODES:
            values["meta"] = {"marker": short}
        calls.append((short, "defaults, positional", list(values.values()), {}))
        calls.append((short, "defaults, keyword", [], dict(values)))
        optional = [p.name for p in inspect.signature(cls.execute).parameters.values() if p.default is not inspect.Parameter.empty]
        for name in optional:
            calls.append((short, f"without {name}", [], {k: v for k, v in values.items() if k != name}))
        if len(optional) > 1:
            calls.append((short, "without " + ", ".join(optional), [], {k: v for k, v in values.items() if k not in optional}))
            calls.append((short, "required sockets positional, the rest left out", list(values.values())[:len(values) - len(optional)], {}))
        for change in HANDOFF_VARIATIONS.get(short, []):
            calls.append((short, "with " + _text(change), [], {**values, **change}))
        if short in APPLY_NODES:
            calls.append((short, "expand, another colour", [values["frames"], values["meta"], "expand", "#102030"], {}))
    return calls


def _apply_frames():
    import torch

    return torch.zeros((2, 4, 6, 3), dtype=torch.float32)


def record_handoff(nodes, short: str, args: list, kwargs: dict) -> dict:
    """One call of a node's `execute` with the module-level hand-on name replaced, as it is looked up at call time."""
    import torch

    cls = getattr(nodes, "VideoStabilizer" + short)
    seen = {}
    if short in ESTIMATOR_NODES:
        def recorder(estimator, *positional, **extras):
            seen.update(estimator=estimator, args=list(positional), extras=extras)
            return "handed on"

        real, nodes._run_estimator_node = nodes._run_estimator_node, recorder
        try:
            assert cls.execute(*args, **kwargs) == "handed on"
        finally:
            nodes._run_estimator_node = real
        return seen

    def recorder(context, meta, rgb, **keywords):
        seen.update(frames=[len(context.frames), context.width, context.height], meta=meta, rgb=rgb, keywords=keywords)
        return SimpleNamespace(frames=torch.full((2, 4, 6, 3), 0.25), masks=torch.ones((2, 4, 6, 1)), meta={"from": "apply_motion"})

    frames = _apply_frames()
    args = [frames if a == "IMAGE:frames" else a for a in args]
    kwargs = {k: frames if v == "IMAGE:frames" else v for k, v in kwargs.items()}
    real, nodes.apply_motion = nodes.apply_motion, recorder
    try:
        out = cls.execute(*args, **kwargs)
    finally:
        nodes.apply_motion = real
    seen["outputs"] = [[list(out[0].shape), float(out[0].mean())], [list(out[1].shape), float(out[1].mean())], out[2]]
    return seen


def dump_handoffs(nodes) -> list:
    return [{"node": short, "case": case, "args": args, "kwargs": kwargs, "record": record_handoff(nodes, short, args, kwargs)}
            for short, case, args, kwargs in _handoff_calls(nodes)]


# ---------------------------------------------------------------- 4. refusals before the GPU

class ContextAsked(Exception):
    """What native.default_context raises here: the call got past every refusal that precedes the GPU work."""


def _frames(n=3, h=6, w=8):
    import torch

    return torch.zeros((n, h, w, 3), dtype=torch.float32)


def _mask(n=3, h=6, w=8, dtype=None):
    import torch

    return torch.zeros((n, h, w), dtype=dtype or torch.float32)


def _meta(n=3, source=(8, 6), output=(8, 6)) -> dict:
    eye = np.eye(3).tolist()
    return {"stabilization_warp": {"per_frame": [{"applied_matrix": eye} for _ in range(n)], "source_size": list(source),
                                   "output_size": list(output)},
            "estimated_motion": {"per_transition": [{"matrix": eye, "confidence": 1.0} for _ in range(n - 1)]},
            "fps_effective": 16.0}


EMPTY_INTAKE = ", behind an intake that lets an empty clip through"


def _refusal_cases() -> dict:
    """"<node>: <what is wrong>" -> (args, kwargs) of its execute.  "A + B" is an input wrong in two ways, which pins which
    refusal comes first; "valid" is refused by nothing and so reaches the context."""
    import torch

    f, m, meta = _frames(), _mask(), _meta()
    no_motion = {"stabilization_warp": meta["stabilization_warp"]}
    i32 = _mask(dtype=torch.int32)
    cases = {}

    def add(node, what, *args, **kwargs):
        assert f"{node}: {what}" not in cases
        cases[f"{node}: {what}"] = (args, kwargs)

    # frames, frames_stabilized, padding_mask, meta, radius, interpolation
    add("TemporalFill", "valid", f, f, m, meta, 8, "bilinear")
    add("TemporalFill", "meta is no dictionary", f, f, m, "meta", 8, "bilinear")
    add("TemporalFill", "meta without transitions", f, f, m, no_motion, 8, "bilinear")
    add("TemporalFill", "unknown interpolation", f, f, m, meta, 8, "nearest")
    add("TemporalFill", "fewer original frames", _frames(2), f, m, meta, 8, "bilinear")
    add("TemporalFill", "more stabilized frames", f, _frames(4), m, meta, 8, "bilinear")
    add("TemporalFill", "original size", _frames(3, 6, 10), f, m, meta, 8, "bilinear")
    add("TemporalFill", "stabilized size", f, _frames(3, 8, 8), m, meta, 8, "bilinear")
    add("TemporalFill", "meta + interpolation", f, f, m, no_motion, 8, "nearest")
    add("TemporalFill", "interpolation + frame count", _frames(2), f, m, meta, 8, "nearest")
    add("TemporalFill", "frame count + size", _frames(2, 6, 10), f, m, meta, 8, "bilinear")
    add("TemporalFill", "empty original clip", [], f, m, meta, 8, "bilinear")
    # ..., feather, match_exposure
    add("TemporalFillBlend", "valid", f, f, m, meta, 8, "bilinear", 16, True)
    add("TemporalFillBlend", "valid, feather 0 without exposure is the plain fill", f, f, m, meta, 8, "bilinear", 0, False)
    add("TemporalFillBlend", "feather is a bool", f, f, m, meta, 8, "bilinear", True, True)
    add("TemporalFillBlend", "feather too wide", f, f, m, meta, 8, "bilinear", 65, True)
    add("TemporalFillBlend", "feather is a float", f, f, m, meta, 8, "bilinear", 8.0, True)
    add("TemporalFillBlend", "match_exposure is no bool", f, f, m, meta, 8, "bilinear", 16, "yes")
    add("TemporalFillBlend", "radius 0", f, f, m, meta, 0, "bilinear", 16, True)
    add("TemporalFillBlend", "feather bool + meta", f, f, m, no_motion, 8, "bilinear", False, True)
    add("TemporalFillBlend", "meta + feather too wide", f, f, m, no_motion, 8, "bilinear", 65, True)
    add("TemporalFillBlend", "feather too wide + interpolation", f, f, m, meta, 8, "nearest", 65, True)
    add("TemporalFillBlend", "interpolation + frame count", _frames(2), f, m, meta, 8, "nearest", 16, True)
    add("TemporalFillBlend", "frame count", _frames(2), f, m, meta, 8, "bilinear", 16, True)
    add("TemporalFillBlend", "stabilized size", f, _frames(3, 8, 8), m, meta, 8, "bilinear", 16, True)
    # frames, frames_stabilized, meta, radius, alpha, padding_mask=None
    add("SharpnessTransfer", "valid", f, f, meta, 2, 16.0)
    add("SharpnessTransfer", "valid, with a mask", f, f, meta, 2, 16.0, m)
    add("SharpnessTransfer", "meta without transitions", f, f, no_motion, 2, 16.0)
    add("SharpnessTransfer", "radius 0", f, f, meta, 0, 16.0)
    add("SharpnessTransfer", "radius 0, no alpha", f, f, meta, 0, None)
    add("SharpnessTransfer", "radius 0, no alpha + frame count", _frames(2), f, meta, 0, None)
    add("SharpnessTransfer", "radius too large", f, f, meta, 17, 16.0)
    add("SharpnessTransfer", "negative alpha", f, f, meta, 2, -1.0)
    add("SharpnessTransfer", "fewer original frames", _frames(2), f, meta, 2, 16.0)
    add("SharpnessTransfer", "more stabilized frames", f, _frames(4), meta, 2, 16.0)
    add("SharpnessTransfer", "original size", _frames(3, 6, 10), f, meta, 2, 16.0)
    add("SharpnessTransfer", "stabilized size", f, _frames(3, 8, 8), meta, 2, 16.0)
    add("SharpnessTransfer", "meta + radius 0", f, f, no_motion, 0, 16.0)
    add("SharpnessTransfer", "radius 0 + frame count", _frames(2), f, meta, 0, 16.0)
    add("SharpnessTransfer", "frame count + size", _frames(2, 6, 10), f, meta, 2, 16.0)
    # frames, padding_mask
    add("PaddingFill", "valid", f, m)
    add("PaddingFill", "valid, one mask for the clip", f, _mask(1))
    add("PaddingFill", "valid, trailing axis", f, m[..., None])
    add("PaddingFill", "valid, numpy float64", f, np.zeros((3, 6, 8)))
    add("PaddingFill", "no frame", _frames(0), _mask(0))
    add("PaddingFill", "mask is None", f, None)
    add("PaddingFill", "mask is a list", f, [[0.0]])
    add("PaddingFill", "integer mask", f, i32)
    add("PaddingFill", "mask [H,W]", f, m[0])
    add("PaddingFill", "mask of two frames", f, _mask(2))
    add("PaddingFill", "mask of another size", f, _mask(3, 6, 9))
    add("PaddingFill", "mask with two channels", f, torch.zeros((3, 6, 8, 2)))
    add("PaddingFill", "no frame + mask is None", _frames(0), None)
    add("PaddingFill", "integer mask + shape", f, i32[:2])
    # frames, padding_mask=None, reference_frames=None
    add("StabilityReport", "valid", f)
    add("StabilityReport", "valid, mask and reference", f, _mask(1), _frames(2))
    add("StabilityReport", "no frame", _frames(0))
    add("StabilityReport", "mask is a list", f, [[0.0]])
    add("StabilityReport", "integer mask", f, i32)
    add("StabilityReport", "mask of two frames", f, _mask(2))
    add("StabilityReport", "mask of another size, trailing axis", f, _mask(3, 7, 8)[..., None])
    add("StabilityReport", "reference without a frame", f, None, _frames(0))
    add("StabilityReport", "reference without a frame, by keyword", f, reference_frames=_frames(0))
    add("StabilityReport", "no frame + integer mask", _frames(0), i32)
    add("StabilityReport", "integer mask + shape", f, i32[:2])
    add("StabilityReport", "mask shape + reference without a frame", f, _mask(2), _frames(0))
    # mask, expand=5, tapered_corners=True, feather=0, hold=0
    add("MaskGrow", "valid", m)
    add("MaskGrow", "valid, [H,W]", m[0], -3, False, 4, 2)
    add("MaskGrow", "expand out of range", m, 65)
    add("MaskGrow", "feather is a bool", m, 5, True, True)
    add("MaskGrow", "hold out of range", m, 5, True, 0, 17)
    add("MaskGrow", "tapered_corners is no bool", m, 5, "yes")
    add("MaskGrow", "mask is a list", [[0.0]])
    add("MaskGrow", "integer mask", i32)
    add("MaskGrow", "mask [N,H,W,1]", m[..., None])
    add("MaskGrow", "mask without a row", _mask(3, 0, 8))
    add("MaskGrow", "expand + mask is a list", [[0.0]], 65)
    add("MaskGrow", "integer mask + shape", i32[..., None])
    # frames, frames_stabilized, padding_mask=None, meta=None, window=1.0, mode="exposure"
    add("Deflicker", "valid, no meta, the clip itself", f, f)
    add("Deflicker", "valid, with a meta", f, _frames(), m, meta, 0.5, "rgb")
    add("Deflicker", "unknown mode", f, f, None, None, 1.0, "luma")
    add("Deflicker", "window 0", f, f, None, None, 0)
    add("Deflicker", "window too long", f, f, None, None, 61.0)
    add("Deflicker", "window None, no mode", f, f, None, None, None, None)
    add("Deflicker", "window False, no mode + one frame", _frames(1), _frames(1), None, None, False, None)
    add("Deflicker", "one frame", _frames(1), _frames(1))
    add("Deflicker", "fewer stabilized frames", f, _frames(2))
    add("Deflicker", "meta without transitions", f, f, None, no_motion)
    add("Deflicker", "meta of another frame count", f, f, None, _meta(4))
    add("Deflicker", "original size", f, f, None, _meta(3, (10, 6), (8, 6)))
    add("Deflicker", "stabilized size", f, _frames(3, 8, 8), None, meta)
    add("Deflicker", "window 0 + one frame", _frames(1), _frames(1), None, None, 0)
    add("Deflicker", "frame count + meta", f, _frames(2), None, no_motion)
    add("Deflicker", "meta frame count + size", f, f, None, _meta(4, (10, 6), (8, 6)))
    # frames, padding_mask=None, fill=True, min_count=1, matte_threshold=0.1, matte_min_count=3
    add("CleanPlate", "valid", f)
    add("CleanPlate", "valid, one mask for the clip", f, _mask(1), False, 2, 0.5, 4)
    add("CleanPlate", "fill is no bool", f, None, 1)
    add("CleanPlate", "min_count 0", f, None, True, 0)
    add("CleanPlate", "min_count is a bool", f, None, True, True)
    add("CleanPlate", "matte_min_count is a float", f, None, True, 1, 0.1, 3.0)
    add("CleanPlate", "matte_threshold above 1", f, None, True, 1, 1.5)
    add("CleanPlate", "matte_threshold is a bool", f, None, True, 1, True)
    add("CleanPlate", "no frame", _frames(0))
    add("CleanPlate", "mask is a list", f, [[0.0]])
    add("CleanPlate", "integer mask", f, i32)
    add("CleanPlate", "mask of two frames", f, _mask(2))
    add("CleanPlate", "fill + min_count", f, None, "yes", 0)
    add("CleanPlate", "min_count + matte_min_count", f, None, True, 0, 0.1, 0)
    add("CleanPlate", "matte_min_count + matte_threshold", f, None, True, 1, 1.5, 0)
    add("CleanPlate", "matte_threshold + no frame", _frames(0), None, True, 1, 1.5)
    add("CleanPlate", "no frame + integer mask", _frames(0), i32)
    add("CleanPlate", "integer mask + shape", f, i32[:2])
    # the intake itself refuses an empty clip (above: "no frame"), so the nodes' own sentence for it is reached only behind an
    # intake that lets one through: record_refusal replaces host_math._normalize_video_input for these four
    add("PaddingFill", "no frame" + EMPTY_INTAKE, f, m)
    add("StabilityReport", "no frame" + EMPTY_INTAKE, f, i32)
    add("StabilityReport", "reference without a frame" + EMPTY_INTAKE, f, None, "REFERENCE")
    add("CleanPlate", "no frame" + EMPTY_INTAKE, f, i32)
    return cases


def record_refusal(nodes, case: str, args, kwargs) -> dict:
    """The exception class and full text with which `case` ends; native.default_context raises ContextAsked."""
    from vstab_amd import native

    def asked(*a, **k):
        raise ContextAsked("the GPU context was asked for")

    def intake(value):   # the frames of the case are a clip of 3 frames; "REFERENCE" is the empty one
        empty = case.startswith("StabilityReport: reference") == (isinstance(value, str) and value == "REFERENCE")
        return SimpleNamespace(frames=[] if empty else [None] * 3, height=6, width=8)

    cls = getattr(nodes, "VideoStabilizer" + case.split(":")[0])
    real, native.default_context = native.default_context, asked
    real_intake = nodes.hm._normalize_video_input
    if case.endswith(EMPTY_INTAKE):
        nodes.hm._normalize_video_input = intake
    try:
        cls.execute(*args, **kwargs)
    except Exception as exc:   # noqa: BLE001 - the class is what is recorded
        return {"type": type(exc).__name__, "text": str(exc)}
    finally:
        native.default_context = real
        nodes.hm._normalize_video_input = real_intake
    return {"type": None, "text": "returned"}


def dump_refusals(nodes) -> dict:
    return {case: record_refusal(nodes, case, args, kwargs) for case, (args, kwargs) in _refusal_cases().items()}


# ---------------------------------------------------------------- the fixture

def dump_surface() -> dict:
    vstab_amd, nodes = _load()
    return {"schemas": dump_schemas(nodes), "registration": dump_registration(vstab_amd, nodes), "handoffs": dump_handoffs(nodes),
            "refusals": dump_refusals(nodes)}


def _serialised(value):
    """What the fixture holds of `value`: tensors and other objects by their repr, tuples as lists."""
    return json.loads(json.dumps(value, default=repr))


@pytest.fixture(scope="module")
def golden() -> dict:
    return json.loads(GOLDEN.read_text())


@pytest.fixture(scope="module")
def api(pkg):
    return _load()


def _same(got, want, what: str) -> None:
    assert _text(got) == _text(want), f"{what} differs from tests/golden/node_surface.json"


def test_schemas_of_all_nodes(api, golden):
    got = dump_schemas(api[1])
    assert list(got) == list(golden["schemas"]) and len(got) == N_NODES
    for name, schema in got.items():
        for key, value in schema.items():
            if key in ("inputs", "outputs"):
                assert [s["id"] for s in value] == [s["id"] for s in golden["schemas"][name][key]], f"{name}: {key}, ids and order"
                for s, want in zip(value, golden["schemas"][name][key]):
                    _same(s, want, f"{name}: socket {s['id']!r} of {key}")
            else:
                _same(value, golden["schemas"][name][key], f"{name}: {key}")


def test_execute_parameters_are_the_input_sockets(api):
    """ComfyUI calls `execute` with the socket ids as keywords: every node's parameters are its inputs, in the schema's order,
    and a parameter may be left out exactly where the fixture says so (test_schemas_of_all_nodes pins the defaults)."""
    for cls in _all_nodes(api[1]):
        assert list(inspect.signature(cls.execute).parameters) == [s.id for s in cls.define_schema().inputs], cls.__name__


def _socket_objects(schema) -> list:
    return list(schema.inputs) + list(schema.outputs)


def test_define_schema_builds_fresh_sockets(api):
    """The host may alter the io objects it is handed: two calls of define_schema() share no socket object, nor do two nodes'
    schemas, nor does a schema hold one twice -- and the lists themselves are fresh."""
    owner, alive = {}, []   # (an id stays unique only while its object lives)
    for cls in _all_nodes(api[1]):
        first, second = cls.define_schema(), cls.define_schema()
        alive += [first, second]
        assert first is not second and first.inputs is not second.inputs and first.outputs is not second.outputs
        assert not {id(s) for s in _socket_objects(first)} & {id(s) for s in _socket_objects(second)}, cls.__name__
        for schema in (first, second):
            for s in _socket_objects(schema):
                assert id(s) not in owner, f"{cls.__name__} shares socket {s!r} with {owner.get(id(s))}"
                owner[id(s)] = cls.__name__
    assert len(owner) == 2 * sum(len(_socket_objects(s)) for s in alive[::2])


def test_registration(api, golden):
    got = dump_registration(*api)
    want = golden["registration"]
    assert len(got["extensions"]) == N_EXTENSIONS and list(got["extensions"]) == list(want["extensions"])
    for name, ext in got["extensions"].items():
        _same(ext, want["extensions"][name], f"extension {name}")
        assert ext["name"] == name
    for key in ("NODE_CLASSES", "entrypoint"):
        _same(got[key], want[key], key)
    assert got["entrypoint"] == "VideoStabilizerAmdMaskedExtension"


def test_what_each_node_hands_on(api, golden):
    """The calls are the fixture's own (written from the schemas and signatures of the tree that wrote it), replayed here."""
    nodes = api[1]
    assert {c["node"] for c in golden["handoffs"]} == set(ESTIMATOR_NODES + APPLY_NODES)
    _same([[n, c, a, k] for n, c, a, k in _handoff_calls(nodes)],
          [[c["node"], c["case"], c["args"], c["kwargs"]] for c in golden["handoffs"]], "the list of hand-on calls")
    records = {}
    for call in golden["handoffs"]:
        got = record_handoff(nodes, call["node"], call["args"], call["kwargs"])
        _same(_serialised(got), call["record"], f"{call['node']}, {call['case']}")
        records[call["node"], call["case"]] = _text(_serialised(got))
    for short in ESTIMATOR_NODES + APPLY_NODES:   # positional and keyword calls are one call
        assert records[short, "defaults, positional"] == records[short, "defaults, keyword"], short
    by = {(c["node"], c["case"]): c["record"] for c in golden["handoffs"]}   # the fixture says what the issue says
    assert by["FlowMesh", "defaults, keyword"]["extras"] == {"mesh_warp": [16, 9], "mesh_max_shift": None}
    assert by["FlowRolling", "defaults, keyword"]["extras"] == {"rolling_shutter": "auto"}
    level = by["FlowLevel", "defaults, keyword"]
    assert _text(level["extras"]) == _text({"horizon_level": True, "horizon_limit": 20.0}) and level["args"][2] == "crop_and_pad"
    exposure = by["FlowAnchoredExposure", 'with {"exclude_mask": "MASK:exclude_mask"}']["extras"]
    assert exposure["drift_mask"] is True and "drift_mask" not in by["FlowAnchoredExposure", "defaults, keyword"]["extras"]


def test_refusals_before_the_gpu(api, golden):
    """116 cases: every `raise` of the eight nodes' `execute` that precedes native.default_context() is hit (30 statements when the
    fixture was written), and so are the refusals of the checks they call; one by one and, where two things are wrong at once, in
    their order.  The 17 "valid" cases end at the context: they show where the line to the GPU work runs."""
    nodes = api[1]
    cases = _refusal_cases()
    assert len(cases) == N_REFUSALS and list(cases) == list(golden["refusals"])
    assert {c.split(":")[0] for c in cases} == set(REFUSING_NODES)
    for case, (args, kwargs) in cases.items():
        got = record_refusal(nodes, case, args, kwargs)
        _same(got, golden["refusals"][case], f"refusal {case!r}")
        assert (got["type"] == "ContextAsked") == case.split(": ")[1].startswith("valid"), f"{case}: {got}"


if __name__ == "__main__":
    if sys.argv[1:] != ["--write"]:
        sys.exit("usage: python tests/test_node_surface_cpu.py --write")
    sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
    GOLDEN.write_text(json.dumps(dump_surface(), indent=1, default=repr) + "\n")
    print(f"wrote {GOLDEN} ({GOLDEN.stat().st_size} bytes)")
