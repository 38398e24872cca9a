#!/usr/bin/env python3
"""Raw bytes of every fit record that two (or more) builds of the library return, compared byte for byte.

For a change of the fit kernels (csrc/vstab_fit.hip, csrc/vstab_homography.hip, csrc/vstab_fit_common.h) that must leave every
bit alone, the homography entries included, which the tests compare to a tolerance only.  A fresh process per library (loaded
through VSTAB_LIB; "-" is the shipped one) dumps every field of the [pairs, 3] record table (FIT_DTYPE) of

  every case of tests/fit_cases.py, with its block grid where it has one      sample_fit_batch
  both point tables of tests/fit_cases.py                                     points_fit_batch
  the bench clip's sampled grid (256 frames of 1080p, 68 x 120 samples)       sample_fit_batch

each in all three requested modes, into DIR/<n>.bin, and prints one line per table (name, mode, records, sha256).  The parent
compares the files: exit status 1 unless all are identical.

    python tools/fit_records_dump.py [--dir DIR] - comfyui-video-stabilizer_amd/lib/libvstab_parent.so
"""
import argparse
import hashlib
import os
import subprocess
import sys
import tempfile
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))


def dump(path):
    import numpy as np
    import torch

    import __graft_entry__ as graft

    graft.load_package()
    import bench
    from tests import fit_cases as C
    from vstab_amd import native

    def cuda(a):
        return torch.from_numpy(np.array(a)).cuda()

    ctx = native.Context(0)
    tables = []
    for case_id in C.CASE_IDS:
        grid, blocked = C.inputs(case_id)
        for mode in C.MODES:
            b = None if blocked is None else cuda(blocked)
            tables.append((case_id, mode, ctx.sample_fit_batch(cuda(grid), C.CASES[case_id].step, mode, blocked=b)))
    for cap in C.POINT_CAPS:
        table, counts, _ = C.point_table(cap)
        for mode in C.MODES:
            tables.append((f"points-{cap}", mode, ctx.points_fit_batch(cuda(table), cuda(counts), mode)))
    frames = bench.synth_clip(256, 0, 1080, 1920, torch.device("cuda", 0))
    gray = ctx.gray_downscale(frames, (960, 540))
    _, grid = ctx.dis_flow_batch(gray, sample_step=8, want_full=False, want_grid=True)
    print("bench-clip grid", tuple(grid.shape), hashlib.sha256(grid.cpu().numpy().tobytes()).hexdigest())
    for mode in C.MODES:
        tables.append(("bench-clip", mode, ctx.sample_fit_batch(grid, 8, mode)))
    with open(path, "wb") as fh:
        for name, mode, table in tables:
            # field by field: the padding inside a record is whatever the device buffer held before
            raw = b"".join(np.ascontiguousarray(table[f]).tobytes() for f in table.dtype.names)
            fh.write(raw)
            print(name, mode, table.size, hashlib.sha256(raw).hexdigest())
    print("tables", len(tables), "records", sum(t.size for _, _, t in tables), "bytes", os.path.getsize(path))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dir", default=None, help="where the dumps go (default: a new temporary directory)")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("libs", nargs="*", help='libraries, relative to the repository root; "-" is the shipped one')
    args = ap.parse_args()
    if args.child:
        dump(args.child)
        return
    out = Path(args.dir or tempfile.mkdtemp(prefix="fit_records_"))
    out.mkdir(parents=True, exist_ok=True)
    print("dumps in", out)
    dumps = []
    for n, lib in enumerate(args.libs or ["-"]):
        env = dict(os.environ)
        if lib != "-":
            env["VSTAB_LIB"] = str(ROOT / lib)
        path = out / f"{n}.bin"
        print(f"== {lib}", flush=True)
        # a child that hangs ends the run (TimeoutExpired): nothing more is started on the GPU after it
        proc = subprocess.run([sys.executable, __file__, "--child", str(path)], env=env, capture_output=True, text=True, timeout=300)
        (out / f"{n}.txt").write_text(proc.stdout)
        print(proc.stdout[-400:] if proc.returncode == 0 else proc.stdout[-2000:] + proc.stderr[-4000:], flush=True)
        if proc.returncode != 0:
            sys.exit(proc.returncode if proc.returncode > 0 else 3)   # nothing more is started after a failed child
        dumps.append(path.read_bytes())
    same = all(d == dumps[0] for d in dumps)
    print(f"{len(dumps)} dumps of {len(dumps[0])} bytes:", "byte-identical" if same else "DIFFERENT (diff the .txt files)")
    sys.exit(0 if same else 1)


if __name__ == "__main__":
    main()
