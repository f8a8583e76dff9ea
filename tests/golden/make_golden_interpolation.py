#!/usr/bin/env python
"""Generates tests/golden/interpolation.npz by IMPORTING the reference's Python (read-only, /root/reference) in the build container, as
make_golden_pose_sequence.py does: stage 4, the poses of the held-out frames inside the dynamic phases,

    trainers.interpolate_pose.decompose_transform    (:28-63)    on seeded transforms for n = 2, 3, 5, 8, 16, 32, a small motion at n = 2 (the
                                                                 descent has not converged after its 1500 steps), a pure translation, the identity
    trainers.interpolate_pose.interpolate_pose_seq   (:65-114)   once, on a seeded sequence with two adjacent dynamic phases: a key before the
                                                                 phases, an old key without a pose, held-out frames, the first frame of the second
                                                                 phase held out (the walk loses it), a trailing run without a pose that ends at an old
                                                                 key without one, old keys past the last phase

run on the CPU (about 3 s per descent).  Scene, GaussianModel, torch.load and save_poses_securely of trainers.interpolate_pose are replaced by
stand-ins that supply the frame names and the old sequence and catch the result.  Only the recorded tensors and names are committed.
Run:  python tests/golden/make_golden_interpolation.py
"""
import os
import sys
import tempfile
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg                                    # noqa: E402  (stub, CudaToCpu, the recording rasterizer)

FRAMES = [f"{i:05d}" for i in range(37)]
PHASES = [("00010", "00020"), ("00021", "00030")]
OLD_KEYS = ["00005", "00010", "00012", "00013", "00016", "00017", "00020", "00024", "00025", "00028", "00031", "00033", "00035"]
OLD_NONE = ["00016", "00031"]


def axis_angle(rng, amax):
    axis = rng.normal(size=3); axis /= np.linalg.norm(axis)
    a = rng.uniform(0.5 * amax, amax)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(a) * K + (1 - np.cos(a)) * (K @ K)


def main():
    mg.stub("plyfile", PlyData=object, PlyElement=object)
    mg.stub("pytorch3d")
    mg.stub("pytorch3d.transforms", euler_angles_to_matrix=None)
    mg.stub("simple_knn")
    mg.stub("simple_knn._C", distCUDA2=lambda pts: torch.full((pts.shape[0],), 1e-3))
    mg.install_recording_rasterizer()
    npy = mg.npy

    with mg.CudaToCpu():
        import trainers.interpolate_pose as ip

        rng = np.random.default_rng(4104)
        f32 = lambda a: torch.tensor(np.asarray(a), dtype=torch.float32)
        # ---- decompose_transform ----
        cases = [("small_n2", 2, axis_angle(rng, 0.01), rng.uniform(-0.01, 0.01, 3))]
        for n in (2, 3, 5, 8, 16, 32):
            cases.append((f"n{n}", n, axis_angle(rng, 0.3), rng.uniform(-0.3, 0.3, 3)))
        cases.append(("translation_n5", 5, np.eye(3), rng.uniform(-0.3, 0.3, 3)))
        cases.append(("identity_n3", 3, np.eye(3), np.zeros(3)))
        out = dict(dec_names=np.array([c[0] for c in cases]), dec_n=np.array([c[1] for c in cases], dtype=np.int64))
        Ts, ts, Rs = [], [], []
        for name, n, R, t in cases:
            T = ip.to_transform_mat(f32(t), f32(R))
            got = ip.decompose_transform(T, n)
            assert len(got) == n and all(g is got[0] or (torch.equal(g["translation"], got[0]["translation"]) and torch.equal(g["rotation"], got[0]["rotation"])) for g in got)
            Ts.append(npy(T)); ts.append(npy(got[0]["translation"])); Rs.append(npy(got[0]["rotation"]))
            print(name, n, ts[-1])
        out.update(dec_T=np.stack(Ts), dec_t=np.stack(ts), dec_R=np.stack(Rs))

        # ---- interpolate_pose_seq ----
        old = {}
        for k in OLD_KEYS:
            old[k] = None if k in OLD_NONE else {"translation": f32(rng.uniform(-0.2, 0.2, 3)), "rotation": f32(axis_angle(rng, 0.2))}
        caught = {}

        class Scene:
            def __init__(self, *a, **kw):
                pass

            def getTrainCameras(self):
                order = rng.permutation(len(FRAMES))                 # (handed over shuffled: the routine sorts)
                return [types.SimpleNamespace(image_name=FRAMES[i]) for i in order]

        class TorchWithLoad:
            def __getattr__(self, name):
                return getattr(torch, name)

            @staticmethod
            def load(path, *a, **kw):
                return dict(old)

        def catch(d, save_dir):
            caught.update(d)
            caught["__order__"] = list(d.keys())
            return os.path.join(save_dir, "obj_pose_sequence.pth")

        ip.Scene, ip.GaussianModel, ip.torch, ip.save_poses_securely = Scene, (lambda *a, **kw: None), TorchWithLoad(), catch
        with tempfile.TemporaryDirectory() as tmp:
            ip.interpolate_pose_seq(types.SimpleNamespace(sh_degree=0), None, None, "golden", tmp, [list(p) for p in PHASES], "unused.pth")
        new_keys = caught.pop("__order__")
        eye_t, eye_R = np.zeros(3, np.float32), np.eye(3, dtype=np.float32)
        pack = lambda d, keys: (np.array([d[k] is not None for k in keys]),
                                np.stack([npy(d[k]["translation"]) if d[k] is not None else eye_t for k in keys]),
                                np.stack([npy(d[k]["rotation"]) if d[k] is not None else eye_R for k in keys]))
        out.update(run_frames=np.array(FRAMES), run_phases=np.array(PHASES), run_old_keys=np.array(OLD_KEYS), run_new_keys=np.array(new_keys))
        out["run_old_valid"], out["run_old_t"], out["run_old_R"] = pack(old, OLD_KEYS)
        out["run_new_valid"], out["run_new_t"], out["run_new_R"] = pack(caught, new_keys)
        print("new keys", new_keys, "valid", out["run_new_valid"].astype(int).tolist())
        path = os.path.join(HERE, "interpolation.npz")
        np.savez_compressed(path, **out)
    print("interpolation.npz", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
