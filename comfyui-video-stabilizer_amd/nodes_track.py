"""The template track's node (template_track.py): the Flow node locked on one box.

A module of its own: nodes.py's namespace -- its node and extension classes -- is what the node surface's fixture lists, so the
node and its extension are made here from nodes.py's own pieces (`_FlowVariant`, `_extend`) and nothing is added there.
`comfy_entrypoint()` and `NODE_CLASSES` are unchanged; an integrator who wants the node registers
`VideoStabilizerAmdTrackExtension`.
"""

from __future__ import annotations

from . import nodes
from . import template_track
from .comfy_compat import io


class VideoStabilizerFlowTrack(nodes._FlowVariant):
    """The Flow node locked on a box: the rectangle (`box_x`, `box_y`, `box_width`, `box_height`) around the subject in frame
    `key_frame` is followed through the clip by a fixed-template search on the estimation images (template_track.py), and the
    box's path -- not the camera's motion -- is what the trajectory steadies: with Camera Lock the subject stays where frame
    0 shows it.  Translation only.  Not one of the reference's nodes: it is listed by an extension but kept out of
    NODE_CLASSES."""

    NODE = ("video_stabilizer_flow_track", "Video Stabilizer Flow (Track Box)",
            "Video Stabilizer Flow that stabilizes on the content of one rectangle drawn in one frame: the subject is "
            "held still (Camera Lock) or followed smoothly, without a segmentation mask.")
    ESTIMATOR = template_track.ESTIMATOR
    FIXED = {"transform_mode": "translation"}

    @staticmethod
    def sockets() -> list:
        big = 1 << 20
        return [
            io.Int.Input("box_x", default=0, min=0, max=big, display_name="Box X",
                         tooltip="Left edge of the rectangle around the subject, in pixels of the frames."),
            io.Int.Input("box_y", default=0, min=0, max=big, display_name="Box Y",
                         tooltip="Top edge of the rectangle around the subject, in pixels of the frames."),
            io.Int.Input("box_width", default=128, min=1, max=big, display_name="Box Width",
                         tooltip="Width of the rectangle, in pixels of the frames (at least 8 pixels of the estimation image)."),
            io.Int.Input("box_height", default=128, min=1, max=big, display_name="Box Height",
                         tooltip="Height of the rectangle, in pixels of the frames (at least 8 pixels of the estimation image)."),
            io.Int.Input("key_frame", default=0, min=0, max=big, display_name="Key Frame",
                         tooltip="The frame the rectangle was drawn in; the clip is tracked forwards and backwards from it."),
            io.Int.Input("search_radius", default=template_track.DEFAULT_RADIUS, min=1, max=48, display_name="Search Radius",
                         tooltip=("How far the subject may move from one frame to the next, in pixels of the estimation image "
                                  "(long side 960).")),
        ]

    @staticmethod
    def extras(box_x, box_y, box_width, box_height, key_frame=0, search_radius=template_track.DEFAULT_RADIUS) -> dict:
        return dict(track_box=(int(box_x), int(box_y), int(box_width), int(box_height)), track_key=int(key_frame),
                    track_radius=int(search_radius))


VideoStabilizerAmdTrackExtension = nodes._extend(
    getattr(nodes, nodes._EXTENSION_CHAIN[-1][0]), VideoStabilizerFlowTrack, name="VideoStabilizerAmdTrackExtension",
    doc="The nodes of the chain's last extension plus Video Stabilizer Flow (Track Box).")
