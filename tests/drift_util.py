"""What the drift-correction GPU tests and tools/drift_correction_report.py share: the clip sizes, the reference's arguments, one
call of the pipeline and the error of a chain of reported transitions against the analytic camera path."""

import numpy as np

ARGS = (False, 0.7, 0.5, 0.6, (127, 127, 127), 16.0)        # camera_lock, strength, smooth, keep_fov, padding, fps
LOCK_ARGS = (True, 1.0, 0.5, 0.6, (127, 127, 127), 16.0)
W, H, N = 960, 540, 64


def stabilize(ctx, frames, mode, args=ARGS, framing="crop_and_pad", **kw):
    from vstab_amd import flow_pipeline as fp
    from vstab_amd import host_math as hm

    return fp._stabilize_frames(hm._normalize_video_input(frames), framing, mode, *args, ctx=ctx, keep_on_device=True, **kw)


def chain_error(meta, cam, w=W, h=H):
    """Centre and worst-corner distance (working px: 960x540 is its own working size) between the chain of the reported
    transitions and cam[i] cam[0]^-1, the worst over EVERY frame."""
    pts = np.array([[w / 2, h / 2, 1.0], [0, 0, 1.0], [w - 1, 0, 1.0], [0, h - 1, 1.0], [w - 1, h - 1, 1.0]]).T
    acc = np.eye(3)
    centre = corner = 0.0
    inv0 = np.linalg.inv(cam[0])
    for i, t in enumerate(meta["estimated_motion"]["per_transition"]):
        acc = np.asarray(t["matrix"], np.float64) @ acc
        d = np.hypot(*((acc @ pts)[:2] - (cam[i + 1] @ inv0 @ pts)[:2]))
        centre, corner = max(centre, float(d[0])), max(corner, float(d[1:].max()))
    return centre, corner
