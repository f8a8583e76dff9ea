#!/usr/bin/env python
"""Generates tests/golden/pose_sequence.npz by IMPORTING the reference's Python (read-only, /root/reference) in the build container, as
make_golden_motion.py does: the object stages' pose bookkeeping,

    utils.geometry_utils.get_accum_T_seq / get_accum_R_seq   (:152-186)  on a seeded 7-key sequence, once with one None entry, once with none
    utils.geometry_utils.rot6d_to_matrix                     (:69-89)    with autograd gradients of sum(w * R) for seeded inputs
    GaussianModel.apply_trans_rot_new                        (scene/gaussian_model.py:939-986)  the (trainable, fixed_T, fixed_R) triples for
                                                             frames before, at, between and past the keys, during_training on and off

run on the CPU.  Only the recorded tensors are committed.  Run:  python tests/golden/make_golden_pose_sequence.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg                                    # noqa: E402  (stub, CudaToCpu, the recording rasterizer)
from make_golden_rotcov import rot                          # noqa: E402

KEYS = ["00020", "00030", "00040", "00050", "00060", "00070", "00080"]
NONE_KEY = "00050"
FRAMES = ["00010", "00020", "00035", "00040", "00055", "00080", "00090"]       # before, at the first, between, at, between, at the last, past


def main():
    mg.stub("plyfile", PlyData=object, PlyElement=object)
    mg.stub("pytorch3d")
    mg.stub("pytorch3d.transforms", euler_angles_to_matrix=None)
    mg.stub("simple_knn")
    mg.stub("simple_knn._C", distCUDA2=lambda pts: torch.full((pts.shape[0],), 1e-3))
    mg.install_recording_rasterizer()
    npy = mg.npy

    with mg.CudaToCpu():
        from scene.gaussian_model import GaussianModel
        from utils.geometry_utils import ObjectMove, get_accum_R_seq, get_accum_T_seq, rot6d_to_matrix

        rng = np.random.default_rng(7117)
        out = dict(keys=np.array(KEYS), none_key=NONE_KEY, frames=np.array(FRAMES))
        seq = {}
        for k in KEYS:
            ang = rng.uniform(-0.3, 0.3, 3)
            seq[k] = {"translation": torch.tensor(rng.uniform(-0.5, 0.5, 3), dtype=torch.float32),
                      "rotation": torch.tensor(rot(*ang), dtype=torch.float32)}
            out["t_" + k], out["R_" + k] = npy(seq[k]["translation"]), npy(seq[k]["rotation"])
        variants = {"full": dict(seq), "gap": {k: (None if k == NONE_KEY else v) for k, v in seq.items()}}
        for name, s in variants.items():
            # (handed over in shuffled key order: the functions sort)
            shuffled = {k: s[k] for k in [KEYS[i] for i in rng.permutation(len(KEYS))]}
            aT, aR = get_accum_T_seq(shuffled), get_accum_R_seq(shuffled)
            for k in KEYS:
                out[f"{name}_has_{k}"] = aT[k] is not None
                if aT[k] is not None:
                    out[f"{name}_accT_{k}"], out[f"{name}_accR_{k}"] = npy(aT[k]), npy(aR[k])

        # the 6-D map and its gradient
        n_r6 = 6
        out["n_r6"] = n_r6
        for i in range(n_r6):
            base = rot(*rng.uniform(-0.3, 0.3, 3))[:, :2] if i else np.eye(3)[:, :2]
            r6 = torch.tensor(base + (rng.normal(size=(3, 2)) * 0.05 if i > 1 else 0.0), dtype=torch.float32, requires_grad=True)
            w = torch.tensor(rng.normal(size=(3, 3)), dtype=torch.float32)
            R = rot6d_to_matrix(r6)
            (R * w).sum().backward()
            out[f"r6_{i}"], out[f"r6_w_{i}"], out[f"r6_R_{i}"], out[f"r6_grad_{i}"] = npy(r6), npy(w), npy(R), npy(r6.grad)

        # the frame rule on the full sequence
        aT, aR = get_accum_T_seq(variants["full"]), get_accum_R_seq(variants["full"])
        N = 8
        t0 = torch.tensor([0.07, -0.11, 0.05])
        r6 = torch.tensor(rot(0.2, -0.1, 0.15)[:, :2], dtype=torch.float32)
        out["obj_translation"], out["obj_rotation_6d"] = npy(t0), npy(r6)
        for frame in FRAMES:
            for training in (False, True):
                g = GaussianModel(0)
                g._xyz = torch.nn.Parameter(torch.tensor(rng.normal(size=(N, 3)).astype(np.float32)))
                g._is_object = torch.ones((N, 1))
                g.trainable_object_move = ObjectMove()
                g.trainable_object_move.obj_translation.data.copy_(t0)
                g.trainable_object_move.obj_rotation_6d.data.copy_(r6)
                p = f"rule_{frame}_{int(training)}_"
                try:
                    triple = g.apply_trans_rot_new(aT, aR, frame, which_object=1, during_training=training)
                except Exception as exc:                    # (none expected; recorded rather than hidden)
                    out[p + "error"] = type(exc).__name__
                    continue
                if triple is None:                          # during training past the last key the reference falls off its loop
                    out[p + "fell_off"] = True
                    continue
                out[p + "has_trainable"], out[p + "has_fixed"] = triple[0] is not None, triple[1] is not None
                if triple[0] is not None:
                    out[p + "cap_t"], out[p + "cap_R"] = npy(triple[0][0]), npy(triple[0][1])
                if triple[1] is not None:
                    out[p + "fixed_T"], out[p + "fixed_R"] = npy(triple[1]), npy(triple[2])
        path = os.path.join(HERE, "pose_sequence.npz")
        np.savez_compressed(path, **out)
    print("pose_sequence.npz", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
