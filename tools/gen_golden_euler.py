#!/usr/bin/env python3
"""Generate tests/golden/euler.npz by running the REFERENCE's own is_rotation_matrix and rotation_matrix_to_euler (src/utils.py:305-347)
on a set of matrices that includes the singular branch (sy < 1e-6), near-singular rotations either side of it, and matrices that are no
rotation.

Run where the reference tree is present:   python tools/gen_golden_euler.py [path to the reference's src directory]
The reference is imported in place; nothing of it is copied, only the arrays it computes are stored.  cv2 is not installed here: a
placeholder module stands in for it (the recipe of tools/gen_golden_global_motion.py); the two functions are pure numpy and never call it.
Bytecode writing is disabled so a read-only reference tree is left untouched.
"""
import sys

sys.dont_write_bytecode = True
import os

os.environ["PYTHONDONTWRITEBYTECODE"] = "1"
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(ROOT), "reference", "src")
OUT = os.path.join(ROOT, "tests", "golden", "euler.npz")


def rot(rx, ry, rz):
    cx, sx, cy, sy, cz, sz = np.cos(rx), np.sin(rx), np.cos(ry), np.sin(ry), np.cos(rz), np.sin(rz)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return Rz @ Ry @ Rx


def main():
    sys.modules.setdefault("cv2", types.ModuleType("cv2"))
    sys.path.insert(0, REF)
    import utils as ref_utils

    rng = np.random.default_rng(11)
    h = np.pi / 2
    mats = [np.eye(3), rot(0.1, -0.15, 0.12), rot(-3.0, 1.2, 2.9), rot(0.0, 0.0, np.pi), rot(np.pi, 0.0, 0.0)]
    mats += [rot(*rng.uniform(-np.pi, np.pi, 3)) for _ in range(24)]
    # the singular branch and its neighbourhood: pitch of +-90 degrees exactly, and off it by less and by more than the 1e-6 of sy
    for s in (1.0, -1.0):
        for d in (0.0, 1e-9, 4e-7, 9.9e-7, 1.01e-6, 2e-6, 1e-4):
            for rx, rz in ((0.3, -0.7), (-2.0, 1.1), (0.0, 0.0)):
                mats.append(rot(rx, s * (h - d), rz))
    # the singular branch exactly (R00 = R10 = 0 as written, not as cos(pi / 2) rounds)
    for a in (0.0, 0.4, -2.5):
        c, s = np.cos(a), np.sin(a)
        mats.append(np.array([[0.0, s, c], [0.0, c, -s], [-1.0, 0.0, 0.0]]))
        mats.append(np.array([[0.0, -s, -c], [0.0, c, -s], [1.0, 0.0, 0.0]]))
    # float32 rotations (the identity of that dtype is subtracted), and matrices that are no rotation, either side of the 1e-6
    mats += [rot(*rng.uniform(-1, 1, 3)).astype(np.float32) for _ in range(4)]
    not_rot = [np.eye(3) * 2.0, np.zeros((3, 3)), np.eye(3) + 1e-3, rot(0.2, 0.1, 0.3) + 2e-7, rot(0.2, 0.1, 0.3) + 6e-7, rot(0.2, 0.1, 0.3) * (1 + 1e-7),
               np.diag([1.0, 1.0, -1.0]) @ rot(0.5, 0.5, 0.5), np.full((3, 3), np.nan)]
    out, flags = {}, []
    for k, R in enumerate(mats + not_rot):
        ok = ref_utils.is_rotation_matrix(R)
        assert isinstance(ok, (bool, np.bool_))
        flags.append(bool(ok))
        out[f"R{k}"] = R
        if ok:
            e = ref_utils.rotation_matrix_to_euler(R)
            assert e.shape == (3,)
            out[f"euler{k}"] = e
    flags = np.array(flags)
    sing = [k for k in range(len(flags)) if flags[k] and np.sqrt(out[f"R{k}"][0, 0] ** 2 + out[f"R{k}"][1, 0] ** 2) < 1e-6]
    assert len(sing) >= 8 and (~flags).sum() >= 4 and flags[:len(mats) - 4].all()
    out["is_rotation"] = flags
    out["singular"] = np.array(sing, np.int64)
    np.savez_compressed(OUT, **out)
    print(OUT, os.path.getsize(OUT), "bytes;", len(flags), "matrices,", len(sing), "on the singular branch,", int((~flags).sum()), "no rotation")


if __name__ == "__main__":
    main()
