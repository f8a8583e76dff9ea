"""The object pose sequence: the table the object stages keep per dynamic frame, resident on the device, and its torch statement.

The reference trains ONE pose pair (ObjectMove: obj_translation, obj_rotation_6d) per dynamic frame on top of the pose accumulated over the
earlier keys, stores the result under the frame's key and rebuilds the accumulated sequences, all on the host and on every iteration
(/root/reference/trainers/fine_obj.py:97-126,216-224, trainers/coarse_obj_pose.py:196-221, utils/geometry_utils.py:69-89,152-186).  Here

    PoseSequence       owns the table on the device -- rel [K,12], valid [K], accum [K,12], the pose [9] and ITS one Adam state -- and
                       launches the two one-wave kernels of csrc/pose_seq.hip around a rasterizer step: head() composes the frame's pose
                       into the buffers the rasterizer reads, tail() turns dL/dA12, dL/dM9 into the pose's Adam step, writes the frame's
                       row and re-accumulates the rows after it.  graph.GraphedTrainStep(pose_sequence=) captures both.
    the torch mirror   rot6d_to_matrix, compose_from_rows, accumulate, tail_step: the same formulas as tensor expressions on any device
                       and in any float type -- the CPU tests' subject, the GPU tests' float32 yardstick and float64 anchor; the role
                       losses.py and motion.py play for their kernels.
    stage 4            PoseSequence.interpolated(): the table with a row for every held-out frame inside the dynamic phases
                       (/root/reference/trainers/interpolate_pose.py) -- interpolation_plan is the reference's bookkeeping on ints,
                       egs_pose_interpolate runs its 1500-step descent for every gap in one launch, decompose_transform is that descent's
                       torch statement with the gradient written out.

Rows.  A frame is described to the kernels by the word (fixed_row, train_row, reload, 0) of int32, read from DEVICE memory: fixed_row is
the table row whose accumulated pose lies under the frame (-1: the identity), train_row the row the trainable pose is stored to (-1: a
fixed-pose frame -- nothing is trained, the pose's Adam state does not move), reload != 0 makes the row's stored pose the parameters first
(fine_obj's `.data` reload; the coarse stage passes 0).  rows() is motion.select_motion's rule on the table's current validity.
"""
import torch

from . import lib as _lib
from . import _hip

NORM_FLOOR = 1e-12                      # F.normalize's eps
BETAS, EPS = (0.9, 0.999), 1e-15        # the stages' Adam (optim.py)


# ---- the torch mirror ---------------------------------------------------------------------------------------------------------------
def _normalize(v):
    return v / v.norm().clamp_min(NORM_FLOOR)


def rot6d_to_matrix(r6):
    """The reference's 6-D map (utils/geometry_utils.py:69-89) for one (3,2) -- or flat [6], row-major -- input: normalise the first
    column, Gram-Schmidt the second, cross product; R's columns are b1, b2, b3.  Differentiable."""
    r6 = r6.reshape(3, 2)
    a1, a2 = r6[:, 0], r6[:, 1]
    b1 = _normalize(a1)
    b2 = _normalize(a2 - (b1 * a2).sum() * b1)
    b3 = torch.linalg.cross(b1, b2)
    return torch.stack((b1, b2, b3), dim=-1)


def _row(accum, row):
    """(A_f [3,3], b_f [3]) of accum[row], the identity for row < 0."""
    if row < 0:
        return torch.eye(3, dtype=accum.dtype, device=accum.device), torch.zeros(3, dtype=accum.dtype, device=accum.device)
    T = accum[row].reshape(3, 4)
    return T[:, :3], T[:, 3]


def compose_from_rows(accum, pose, fixed_row, train_row):
    """What egs_pose_head writes: (A12 [3,4], M [3,3]).  train_row < 0: accum[fixed_row] and its rotation block as they are (the identity
    for fixed_row < 0).  Else R_t = rot6d_to_matrix(pose[3:9]), A = R_t A_f, b = R_t b_f + pose[0:3], M = R_t R_f with R_f = A_f --
    motion.ObjectMotion(fixed_T, module).compose().  Differentiable w.r.t. `pose`."""
    A, b = _row(accum, fixed_row)
    if train_row < 0:
        return torch.cat([A, b[:, None]], dim=1), A.clone()
    Rt = rot6d_to_matrix(pose[3:9])
    A2 = Rt @ A
    return torch.cat([A2, (Rt @ b + pose[0:3])[:, None]], dim=1), A2.clone()


def accumulate(rel, valid, start=0, accum=None):
    """accum [K,12]: row k = [A | b] of T_k ... T_1 over the valid rows (get_accum_T_seq; its rotation block is get_accum_R_seq's entry);
    an invalid row repeats its predecessor, a row before any valid one is the identity.  start > 0 (with `accum`): rows below `start` are
    kept, the chain continues from row start - 1."""
    K = rel.shape[0]
    out = torch.zeros((K, 12), dtype=rel.dtype, device=rel.device) if accum is None else accum.clone()
    carry = torch.eye(4, dtype=rel.dtype, device=rel.device)
    if start > 0:
        carry[:3] = out[start - 1].reshape(3, 4)
    for k in range(start, K):
        if bool(valid[k]):
            T = torch.eye(4, dtype=rel.dtype, device=rel.device)
            T[:3] = rel[k].reshape(3, 4)
            carry = T @ carry
        out[k] = carry[:3].reshape(12)
    return out


def pose_gradient(accum, pose, grad21, fixed_row):
    """dL/dpose [9] from grad21 = (dL/dA12 [12], dL/dM9 [9]): dL/dt = dL/db, dL/dR_t = dL/dA A_f^T + dL/db b_f^T + dL/dM R_f^T, then back
    through the 6-D map -- written out (no autograd), the formulas of csrc/pose_seq.hip."""
    A, b = _row(accum, fixed_row)
    gA12, gM = grad21[:12].reshape(3, 4), grad21[12:21].reshape(3, 3)
    gA, gb = gA12[:, :3], gA12[:, 3]
    G = gA @ A.t() + gb[:, None] * b[None, :] + gM @ A.t()
    return torch.cat([gb, rot6d_backward(pose[3:9], G)])


def rot6d_backward(r6, G):
    """dL/dr6 [6] (r6's row-major layout) from G = dL/dR [3,3] of R = rot6d_to_matrix(r6), written out."""
    r6 = r6.reshape(3, 2)
    a1, a2 = r6[:, 0], r6[:, 1]
    n1 = a1.norm().clamp_min(NORM_FLOOR)
    b1 = a1 / n1
    d = (b1 * a2).sum()
    u = a2 - d * b1
    n2 = u.norm().clamp_min(NORM_FLOOR)
    b2 = u / n2
    g1, g2, g3 = G[:, 0], G[:, 1], G[:, 2]
    g1 = g1 + torch.linalg.cross(b2, g3)
    g2 = g2 + torch.linalg.cross(g3, b1)

    def back(y, n, gy):
        c = (y * gy).sum() if float(n) > NORM_FLOOR else torch.zeros((), dtype=y.dtype, device=y.device)
        return (gy - y * c) / n
    gu = back(b2, n2, g2)
    gd = -(gu * b1).sum()
    ga2 = gu + gd * b1
    g1 = g1 + gd * a2 - d * gu
    ga1 = back(b1, n1, g1)
    return torch.stack((ga1, ga2), dim=-1).reshape(6)


def tail_step(accum, rel, valid, pose, exp_avg, exp_avg_sq, step, lr, grad21, fixed_row, train_row, betas=BETAS, eps=EPS):
    """What egs_pose_tail does, out of place -> dict(dpose, pose, exp_avg, exp_avg_sq, step, rel, valid, accum).  train_row < 0: every
    state tensor comes back as it is (dpose None).  step, lr: [2], translation then rotation.  The Adam step is torch.optim.Adam's
    (weight_decay 0, no amsgrad): m += (1 - b1)(g - m); v = b2 v + (1 - b2) g^2; p -= lr / (1 - b1^t) * m / (sqrt(v) / sqrt(1 - b2^t) + eps)."""
    if train_row < 0:
        return dict(dpose=None, pose=pose, exp_avg=exp_avg, exp_avg_sq=exp_avg_sq, step=step, rel=rel, valid=valid, accum=accum)
    g = pose_gradient(accum, pose, grad21, fixed_row)
    b1, b2 = betas
    new_step = step + 1
    st = torch.cat([new_step[0:1].expand(3), new_step[1:2].expand(6)]).to(torch.float64)
    lr9 = torch.cat([lr[0:1].expand(3), lr[1:2].expand(6)]).to(torch.float64)
    ss = (lr9 / (1.0 - b1 ** st)).to(pose.dtype)
    ib = (1.0 / torch.sqrt(1.0 - b2 ** st)).to(pose.dtype)
    m = exp_avg + (1.0 - b1) * (g - exp_avg)
    v = b2 * exp_avg_sq + (1.0 - b2) * g * g
    p = pose - ss * (m / (v.sqrt() * ib + eps))
    rel2, valid2 = rel.clone(), valid.clone()
    rel2[train_row] = torch.cat([rot6d_to_matrix(p[3:9]), p[0:3, None]], dim=1).reshape(12)
    valid2[train_row] = 1
    return dict(dpose=g, pose=p, exp_avg=m, exp_avg_sq=v, step=new_step, rel=rel2, valid=valid2,
                accum=accumulate(rel2, valid2, start=train_row, accum=accum))


# ---- stage 4: the poses of the held-out dynamic frames (/root/reference/trainers/interpolate_pose.py) -----------------------------------
GAP_MIN, GAP_MAX = 2, 32
DESCENT_ITERS, DESCENT_LR = 1500, 0.01      # decompose_transform's epochs and SGD lr
RESIDUAL_FACTOR = 3.0                       # x the float32 mirror's figure: the factor of the float32 yardsticks in tests/anchors.py
RESIDUAL_FLOOR = 2.0 * 2.0 ** -23           # ... and never below two float32 ulps of 1: a float32 product can hit T exactly


def _gap_length(n):
    n = int(n)
    if n < GAP_MIN or n > GAP_MAX:
        raise ValueError(f"pose interpolation: a gap of {n} frames is outside [{GAP_MIN}, {GAP_MAX}] -- below 2 there is nothing to split; the "
                         "reference's descent (lr 0.01 on the mean over 16 entries) has step x curvature of about 0.00125 n^2, which reaches "
                         "2 at n = 40: from 40 frames on it diverges (final loss 1.7 at 40, NaN at 48) and there is no behaviour to reproduce; "
                         "33 to 39 is not characterised")
    return n


def _homogeneous(R, t):
    M = torch.eye(4, dtype=R.dtype, device=R.device)
    M[:3, :3], M[:3, 3] = R, t
    return M


def _chain(M, n):
    """[M, M M, ..., M^n] as the reference builds its product: left to right, n factors."""
    out = [M]
    for _ in range(1, n):
        out.append(out[-1] @ M)
    return out


def descent_gradient(t, r6, T, n):
    """(P = M^n, dL/dt [3], dL/dr6 [6]) of L = mean over the 16 entries of (M^n - T)^2, M = [R(r6) | t; 0 0 0 1], written out: all n
    factors are the same matrix, so dL/dM = sum_k (M^(k-1))^T G (M^(n-k))^T with G = 2 (P - T) / 16; its rotation block goes back through
    the 6-D map (rot6d_backward), its last column is dL/dt."""
    M = _homogeneous(rot6d_to_matrix(r6), t)
    powers = _chain(M, n)
    P = powers[-1]
    S = torch.stack([torch.eye(4, dtype=M.dtype, device=M.device)] + powers[:-1])          # S[j] = M^j, j = 0 .. n - 1
    dM = (S.transpose(1, 2) @ ((P - T) * (2.0 / 16.0)) @ S.flip(0).transpose(1, 2)).sum(0)
    return P, dM[:3, 3], rot6d_backward(r6, dM[:3, :3])


def decompose_transform(T, n, dtype=torch.float32, iters=DESCENT_ITERS, lr=DESCENT_LR):
    """The reference's decompose_transform (interpolate_pose.py:28-63) as tensor expressions with the analytic gradient ->
    (translation [3], rotation [3,3], residual).  From t = 0, r6 = I[:, :2]: `iters` plain gradient steps of size lr on the mean over all
    16 entries of (M^n - T)^2; the loop leaves AFTER the step at which isclose(M^n, T, rtol=1e-7, atol=1e-9) held on every entry of the
    product computed before that step.  The result is the END POINT (t, R(r6)) -- for a short gap and a small motion the descent has
    not converged, and the end point is what the later stages consume; residual = max |M^n - T| of it.  T: a 4x4 transform (or a 3x4
    [R | t] block), any device; n outside [2, 32]: ValueError."""
    n = _gap_length(n)
    T = torch.as_tensor(T).detach().to(dtype)
    if tuple(T.shape) == (3, 4) or T.numel() == 12:
        T = torch.cat([T.reshape(3, 4), torch.tensor([[0.0, 0.0, 0.0, 1.0]], dtype=dtype, device=T.device)])
    T = T.reshape(4, 4)
    t = torch.zeros(3, dtype=dtype, device=T.device)
    r6 = torch.eye(3, dtype=dtype, device=T.device)[:, :2].reshape(6).clone()
    for _ in range(int(iters)):
        P, gt, g6 = descent_gradient(t, r6, T, n)
        done = bool(torch.isclose(P, T, rtol=1e-7, atol=1e-9).all())
        t, r6 = t - lr * gt, r6 - lr * g6
        if done:
            break
    R = rot6d_to_matrix(r6)
    return t, R, (_chain(_homogeneous(R, t), n)[-1] - T).abs().max()


def interpolation_plan(keys, valid, frame_names, dynamic_phases):
    """The reference's two passes over the sequence (interpolate_pose.py:83-109) on ints -> (new_keys, carried, gaps).
    keys, valid: the old table's keys and one truth value per key; frame_names: every training frame; dynamic_phases: (first, last)
    frame names, both ends inclusive.  new_keys: the new table's keys, sorted (the entries of frame_names as given); carried: {new row:
    old row} of the rows that keep the old table's entry, valid or not; gaps: [(first_row, n, old_row)] -- n consecutive new rows ending
    at the key old_row of the old table, all n of which receive the same pose, the key included.
    Pass 1 walks the frames in order: an old key is taken over whatever the phases say; any other frame inside the CURRENT phase becomes
    an empty entry; the phase index advances by one after a frame past the current phase's end (after that frame's own test, one phase
    per frame), and the walk ends with the frame that moved it past the last phase -- old keys after it are dropped.  Pass 2 collects
    runs of empty entries (an old key without a pose is one) up to the next key that has a pose; a run with no such key after it stays
    empty."""
    old = {int(k): i for i, k in enumerate(keys)}
    phases = [(int(a), int(b)) for a, b in dynamic_phases]
    if not phases:
        raise ValueError("interpolation_plan: no dynamic phase")
    frames = sorted(frame_names, key=int)
    new_keys, source = [], []                        # source: the old row, or -1 for an empty entry
    phase = 0
    for name in frames:
        f = int(name)
        if f in old:
            new_keys.append(name); source.append(old[f])
        elif phases[phase][0] <= f <= phases[phase][1]:
            new_keys.append(name); source.append(-1)
        if f > phases[phase][1]:
            phase += 1
        if phase > len(phases) - 1:
            break
    carried = {row: src for row, src in enumerate(source) if src >= 0}
    gaps, run = [], []
    for row, src in enumerate(source):
        has_pose = src >= 0 and bool(valid[src])
        if not has_pose:
            run.append(row)
        elif run:
            run.append(row)
            gaps.append((run[0], len(run), src))
            for r in run:
                carried.pop(r, None)
            run = []
    return new_keys, carried, gaps


# ---- the device-resident table --------------------------------------------------------------------------------------------------------
def select_rows(keys, valid, frame_name, during_training=False):
    """motion.select_motion's rule as table rows -> (fixed_row, train_row).  keys: the sorted frame keys as ints; valid: one truth value per
    key.  Before the first key: (-1, -1).  Training: train_row = the first key >= the frame (none: (-1, -1), where the reference falls off
    its loop), fixed_row = the last VALID key strictly before the frame (-1: the identity).  Not training: the frame's key (ValueError
    when that key is invalid), else the last valid key before the frame, else -- past the end -- the last valid key; train_row = -1."""
    name = int(frame_name)
    if name < keys[0]:
        return -1, -1
    at = next((i for i, k in enumerate(keys) if k >= name), None)
    last_valid = lambda end: next((i for i in range(end - 1, -1, -1) if valid[i]), -1)
    if during_training:
        return (-1, -1) if at is None else (last_valid(at), at)
    if at is not None and keys[at] == name:
        if not valid[at]:
            raise ValueError(f"PoseSequence.rows: frame {frame_name} has no pose yet (its key is invalid) and a fixed pose was asked of it")
        return at, -1
    return last_valid(len(keys) if at is None else at), -1


class PoseSequence:
    def __init__(self, keys, device="cpu", betas=BETAS, eps=EPS):
        """keys: the frame names of the sequence (the keys of the reference's obj_pose_sequence); they are sorted by int().  Every entry
        starts invalid (the reference's None), the pose as reset_pose() leaves it, both learning rates 0.  On a HIP device accumulate(),
        head() and tail() are the kernels of csrc/pose_seq.hip; on the CPU accumulate() is the mirror and head() / tail() raise."""
        self.keys = sorted((str(k) for k in keys), key=int)
        self._ints = [int(k) for k in self.keys]
        if not self.keys or len(set(self._ints)) != len(self._ints):
            raise ValueError("PoseSequence: at least one key, no two equal as integers")
        self.K, self.device = len(self.keys), torch.device(device)
        self._index = {k: i for i, k in enumerate(self._ints)}
        self.betas, self.eps = (float(betas[0]), float(betas[1])), float(eps)
        dev = self.device
        self.rel = torch.zeros((self.K, 12), device=dev)
        self.rel[:, 0] = self.rel[:, 5] = self.rel[:, 10] = 1.0
        dev = self.device = self.rel.device                  # ("cuda" -> the current device's index: what every tensor handed in later reports)
        self.valid = torch.zeros(self.K, dtype=torch.uint8, device=dev)
        self.accum = self.rel.clone()
        self.pose = torch.zeros(9, device=dev)
        self.exp_avg, self.exp_avg_sq = torch.zeros(9, device=dev), torch.zeros(9, device=dev)
        self.step, self.lr = torch.zeros(2, device=dev), torch.zeros(2, device=dev)
        self.dpose = torch.zeros(9, device=dev)             # dL/dpose of the last trainable frame: the trainers' "t Grad" / "R Grad"
        self.reset_pose()
        self._struct = None

    # ---- host API ---------------------------------------------------------------------------------------------------------------------
    def index(self, key):
        try:
            return self._index[int(key)]
        except KeyError:
            raise KeyError(f"PoseSequence: {key!r} is not a key of this sequence") from None

    def set(self, key, translation, rotation):
        """Stores key's relative pose: translation [3], rotation [3,3] (or a (3,2) 6-D rotation).  accumulate() afterwards."""
        i = self.index(key)
        rotation = torch.as_tensor(rotation, dtype=torch.float32)
        if tuple(rotation.shape) == (3, 2):
            rotation = rot6d_to_matrix(rotation)
        row = torch.cat([rotation.detach().reshape(3, 3).cpu(), torch.as_tensor(translation, dtype=torch.float32).detach().reshape(3, 1).cpu()], dim=1)
        self.rel[i] = row.reshape(12).to(self.device)
        self.valid[i] = 1

    def clear(self, key):
        """Makes key's entry invalid (the reference's None).  accumulate() afterwards."""
        self.valid[self.index(key)] = 0

    def reset_pose(self):
        """init_obj_pose plus a fresh optimizer: t = 0, the 6-D rotation = the first two columns of I, moments and step counts zero."""
        self.pose.copy_(torch.tensor([0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 1.0, 0.0, 0.0]))
        self.exp_avg.zero_(); self.exp_avg_sq.zero_(); self.step.zero_()

    def set_lr(self, translation=None, rotation=None):
        """The pose's two learning rates, device scalars the tail reads: no re-capture (the stages' zero_pose_lr / restore_pose_lr)."""
        if translation is not None:
            self.lr[0:1].fill_(float(translation))
        if rotation is not None:
            self.lr[1:2].fill_(float(rotation))

    def rows(self, frame_name, during_training=False):
        """(fixed_row, train_row) of a frame by select_rows on the table's CURRENT validity (reads `valid`: synchronises)."""
        return select_rows(self._ints, self.valid.cpu().tolist(), frame_name, during_training)

    def word(self, rows, reload=False):
        """The frame word of (fixed_row, train_row) as a host int32[4] tensor (range-checked: ValueError)."""
        fixed_row, train_row = int(rows[0]), int(rows[1])
        for r in (fixed_row, train_row):
            if r < -1 or r >= self.K:
                raise ValueError(f"PoseSequence.word: row {r} outside [-1, {self.K})")
        return torch.tensor([fixed_row, train_row, int(bool(reload)), 0], dtype=torch.int32)

    def accumulate(self):
        """accum from rel and valid, all rows (after set() / clear())."""
        if self.device.type != "cuda":
            self.accum.copy_(accumulate(self.rel, self.valid))
            return
        with _hip.device_ctx(self.device):
            _lib.check(_lib.load().egs_pose_accumulate(self.struct(), _hip.stream_of(self.device)))

    def export(self):
        """The reference's obj_pose_sequence: {key: {"translation": [3], "rotation": [3,3]} or None}, CPU tensors (save_poses_securely)."""
        rel, valid = self.rel.cpu().reshape(self.K, 3, 4), self.valid.cpu().tolist()
        return {k: ({"translation": rel[i, :, 3].clone(), "rotation": rel[i, :, :3].clone()} if valid[i] else None) for i, k in enumerate(self.keys)}

    def accum_T_seq(self):
        """get_accum_T_seq of export(): {key: 4x4 CPU tensor, None for an invalid key}."""
        acc, valid = self.accum.cpu().reshape(self.K, 3, 4), self.valid.cpu().tolist()
        bottom = torch.tensor([[0.0, 0.0, 0.0, 1.0]])
        return {k: (torch.cat([acc[i], bottom]) if valid[i] else None) for i, k in enumerate(self.keys)}

    def accum_R_seq(self):
        """get_accum_R_seq of export(): {key: 3x3 CPU tensor, None for an invalid key} -- the rotation blocks of accum."""
        acc, valid = self.accum.cpu().reshape(self.K, 3, 4), self.valid.cpu().tolist()
        return {k: (acc[i, :, :3].clone() if valid[i] else None) for i, k in enumerate(self.keys)}

    def interpolated(self, frame_names, dynamic_phases, check=True):
        """Stage 4 (interpolate_pose_seq): a NEW table on the same device whose keys are interpolation_plan's -- the old keys up to the
        end of the last phase plus every other frame of frame_names inside a phase -- with the carried rows copied bit for bit and the
        rows of every gap filled with the end point of the reference's descent: ONE launch of egs_pose_interpolate over all gaps on a
        HIP device, decompose_transform per gap on the CPU.  accumulate() has been run; the pose and its Adam state are fresh (the
        learning rates 0).  .gaps is the plan's list, .gap_residual float32[G] max |M^n - T| per gap.
        check (HIP only; the CPU rows ARE the mirror's): one host read of the residuals; a gap whose residual is not within
        max(RESIDUAL_FACTOR x the residual of its own float32 mirror, RESIDUAL_FLOOR) (decompose_transform on the CPU: about half a second per gap -- pass
        check=False where that matters) is named in a warning.  A gap longer than 32 frames: ValueError, nothing is built."""
        new_keys, carried, gaps = interpolation_plan(self._ints, self.valid.cpu().tolist(), frame_names, dynamic_phases)
        for _, n, _ in gaps:
            _gap_length(n)
        new = PoseSequence(new_keys, self.device, self.betas, self.eps)
        if carried:
            rows = torch.tensor(sorted(carried), device=self.device)
            src = torch.tensor([carried[r] for r in sorted(carried)], device=self.device)
            new.rel[rows], new.valid[rows] = self.rel[src], self.valid[src]
        new.gaps, G = gaps, len(gaps)
        new.gap_residual = torch.zeros(G, device=self.device)
        if G and self.device.type != "cuda":
            for g, (first, n, old_row) in enumerate(gaps):
                t, R, res = decompose_transform(self.rel[old_row], n)
                new.rel[first:first + n] = torch.cat([R, t[:, None]], dim=1).reshape(12)
                new.valid[first:first + n] = 1
                new.gap_residual[g] = res
        elif G:
            words = torch.tensor(gaps, dtype=torch.int32).to(self.device)
            status = torch.zeros(1, dtype=torch.int32, device=self.device)
            with _hip.device_ctx(self.device):
                _lib.check(_lib.load().egs_pose_interpolate(self.struct(), new.struct(), words.data_ptr(), G, DESCENT_ITERS, DESCENT_LR,
                                                            new.gap_residual.data_ptr(), status.data_ptr(), _hip.stream_of(self.device)))
            if check:
                got, rel = new.gap_residual.cpu().tolist(), self.rel.cpu()
                off = []
                for (first, n, old_row), r in zip(gaps, got):
                    bar = max(RESIDUAL_FACTOR * float(decompose_transform(rel[old_row], n)[2]), RESIDUAL_FLOOR)
                    if not r <= bar:
                        off.append(f"frames {new_keys[first]} .. {new_keys[first + n - 1]} (n = {n}): residual {r:.3e} > {bar:.3e}")
                if off:
                    import warnings
                    warnings.warn("PoseSequence.interpolated: the descent of these gaps ended further from its key's pose than "
                                  f"{RESIDUAL_FACTOR:g} x its float32 mirror does: " + "; ".join(off))
        new.accumulate()
        return new

    # ---- the kernels ------------------------------------------------------------------------------------------------------------------
    def struct(self):
        """The egs_pose_sequence of this table (its tensors never move)."""
        if self._struct is None:
            st = _lib.PoseSequence()
            st.K = self.K
            for name in ("rel", "valid", "accum", "pose", "exp_avg", "exp_avg_sq", "step", "lr"):
                setattr(st, name, getattr(self, name).data_ptr())
            st.beta1, st.beta2, st.eps = self.betas[0], self.betas[1], self.eps
            self._struct = st
        import ctypes
        return ctypes.byref(self._struct)

    def _device_arg(self, t, n, dtype, what):
        if not (torch.is_tensor(t) and t.is_cuda and t.device == self.device and t.dtype == dtype and t.numel() == n and t.is_contiguous()):
            raise RuntimeError(f"PoseSequence: {what} is a contiguous {dtype} tensor of {n} elements on {self.device} (the kernels have no CPU path; "
                               "compose_from_rows / tail_step are the torch statement)")
        return t.data_ptr()

    def head(self, word, A12, M9):
        """egs_pose_head: word int32[4] ON THE DEVICE (a view into a packed frame will do), A12 float32[12], M9 float32[9] outputs."""
        if self.device.type != "cuda":
            raise RuntimeError("PoseSequence.head: HIP devices only (compose_from_rows is the torch statement)")
        w, a, m = self._device_arg(word, 4, torch.int32, "word"), self._device_arg(A12, 12, torch.float32, "A12"), self._device_arg(M9, 9, torch.float32, "M9")
        with _hip.device_ctx(self.device):
            _lib.check(_lib.load().egs_pose_head(self.struct(), w, a, m, _hip.stream_of(self.device)))

    def tail(self, word, grad21, dpose=None, skip=None):
        """egs_pose_tail: grad21 float32[21] as the rasterizer's backward leaves it; dpose (default: self.dpose) receives dL/dpose;
        skip: the step's overflow word (uint32 / int32 [1+] on the device) or None."""
        if self.device.type != "cuda":
            raise RuntimeError("PoseSequence.tail: HIP devices only (tail_step is the torch statement)")
        dpose = self.dpose if dpose is None else dpose
        w, g, d = self._device_arg(word, 4, torch.int32, "word"), self._device_arg(grad21, 21, torch.float32, "grad21"), self._device_arg(dpose, 9, torch.float32, "dpose")
        with _hip.device_ctx(self.device):
            _lib.check(_lib.load().egs_pose_tail(self.struct(), w, g, d, None if skip is None else skip.data_ptr(), _hip.stream_of(self.device)))
