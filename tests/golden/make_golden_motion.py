#!/usr/bin/env python
"""Generates tests/golden/motion.npz by IMPORTING the reference's Python (read-only, /root/reference) in the build container: the
per-frame object pose of every stage after the static one,

    gaussians.apply_trans_rot_new(accum_T_seq, accum_R_seq, image_name, which_object=1, during_training)
    gaussians.reverse_trans_rot_new(which_object=1, trainable_t_R, fixed_T, replace_to_optimizer=False)
        /root/reference/scene/gaussian_model.py:939-986,1037-1060, /root/reference/utils/geometry_utils.py:14-33,188-200

run on CPU for a seeded model of N = 64 Gaussians (`_is_object` stored [N,1] as the reference does, row 0 unselected), three keyed
poses and a perturbed ObjectMove.  Six cases hit the six exits of the frame rule: before the first key, on a key, between keys,
past the last key, during_training on a key, during_training between keys.  Stored per case: the returned triple, the moved xyz,
the gradients of sum(w * xyz') w.r.t. _xyz / obj_translation / obj_rotation_6d (seeded w) and the reversed xyz.  Data only.
Run:  python tests/golden/make_golden_motion.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg                                    # noqa: E402  (stub, CudaToCpu, the recording rasterizer)
from make_golden_rotcov import rot                          # noqa: E402


def pose(ax, ay, az, t):
    T = np.eye(4)
    T[:3, :3] = rot(ax, ay, az)
    T[:3, 3] = t
    return torch.tensor(T, dtype=torch.float32)


CASES = [  # name, image_name, during_training
    ("before_first", "00010", False),
    ("on_key", "00030", False),
    ("between_keys", "00035", False),
    ("past_last", "00090", False),
    ("train_on_key", "00030", True),
    ("train_between", "00035", True),
]


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
        from utils.geometry_utils import ObjectMove

        rng = np.random.default_rng(5151)
        N = 64
        xyz0 = rng.normal(size=(N, 3)).astype(np.float32) * 1.5
        is_obj = (rng.uniform(size=(N, 1)) < 0.3).astype(np.float32)
        is_obj[0, 0] = 0.0
        keys = ["00020", "00030", "00040"]
        accum_T = {"00040": pose(0.5, -0.2, 0.9, [0.4, -0.3, 0.2]), "00020": pose(0.1, 0.3, -0.2, [0.1, 0.05, -0.2]),
                   "00030": pose(-0.4, 0.25, 0.6, [-0.2, 0.3, 0.15])}
        accum_R = {k: accum_T[k][:3, :3].clone() for k in keys}
        w = torch.tensor(rng.normal(size=(N, 3)).astype(np.float32))
        t0 = torch.tensor([0.07, -0.11, 0.05])
        r6 = torch.tensor(rot(0.3, -0.2, 0.25)[:, :2] + rng.normal(size=(3, 2)) * 0.05, dtype=torch.float32)   # not orthonormal: the 6-D map works

        out = dict(N=N, xyz=xyz0, is_object=is_obj, which_object=1, w=npy(w), keys=np.array(keys), obj_translation=npy(t0), obj_rotation_6d=npy(r6),
                   cases=np.array([c[0] for c in CASES]), image_names=np.array([c[1] for c in CASES]),
                   during_training=np.array([c[2] for c in CASES]))
        for k in keys:
            out["T_" + k] = npy(accum_T[k]); out["R_" + k] = npy(accum_R[k])

        for name, image_name, training in CASES:
            g = GaussianModel(0)
            leaf = torch.nn.Parameter(torch.tensor(xyz0))
            g._xyz = leaf
            g._is_object = torch.tensor(is_obj)
            g.trainable_object_move = ObjectMove()
            g.trainable_object_move.obj_translation.data.copy_(t0)
            g.trainable_object_move.obj_rotation_6d.data.copy_(r6)
            tom = g.trainable_object_move
            triple = g.apply_trans_rot_new(accum_T, accum_R, image_name, which_object=1, during_training=training)
            p = name + "_"
            out[p + "has_trainable"] = triple[0] is not None
            out[p + "has_fixed"] = triple[1] is not None
            if triple[0] is not None:
                out[p + "cap_t"] = npy(triple[0][0]); out[p + "cap_R"] = npy(triple[0][1])
            if triple[1] is not None:
                out[p + "fixed_T"] = npy(triple[1]); out[p + "fixed_R"] = npy(triple[2])
            moved = g._xyz
            out[p + "moved_xyz"] = npy(moved)
            if moved.requires_grad and moved is not leaf:
                (moved * w).sum().backward()
                out[p + "g_xyz"] = npy(leaf.grad)
                if training:
                    out[p + "g_translation"] = npy(tom.obj_translation.grad); out[p + "g_rotation_6d"] = npy(tom.obj_rotation_6d.grad)
            with torch.no_grad():
                g._xyz = g._xyz.detach()
                g.reverse_trans_rot_new(which_object=1, trainable_t_R=triple[0], fixed_T=triple[1], replace_to_optimizer=False)
                out[p + "reversed_xyz"] = npy(g._xyz)
                print(name, "round trip max err", float((g._xyz - leaf).abs().max()))
        path = os.path.join(HERE, "motion.npz")
        np.savez_compressed(path, **out)
    print("motion.npz", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
