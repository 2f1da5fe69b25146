#!/usr/bin/env python3
"""Loop candidates found: a course flown 1 1/4 times, its revisits found by place recognition on the device.

    python examples/find_loops.py [--lap 64] [--per-step 32] [--words 1024] [--seed 0]

The course is a circle over landmarks that carry ORB descriptor rows.  A frame sees the landmarks within 1.3 steps of its position and
observes each row with up to 10 of its 256 bits flipped; on the second lap the camera passes 0.15 steps beside its first track, so the
frames of the last quarter lap see the ground of the first quarter again, from almost the same place.  Nothing tells the library
which frames those are.  The rows go into frame slots (FrontEnd.set_orb_rows: no image, no detection), a vocabulary is trained on the
first lap (train_vocabulary), every frame becomes one histogram of the keyframe index (places_add), and places_query asks every entry
for the two entries that share the most words with it, at least `min_gap` frames away and with at least `min_shared` words.  Printed:
every candidate beside the ground-truth revisits.  The best candidate then goes where a candidate goes next: the older frame's
landmarks are staged as a map (stage_map) and the newer frame is placed in it by its descriptors (relocalize) — the pose is compared
with the truth."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

VIEW = 2.6             # landmarks within VIEW / 2 steps of the camera are seen
SIDE_STEP = 0.15       # every further lap passes this many steps beside the one before
MAX_FLIPS = 10
CAMERA = np.array([[300.0, 0, 320], [0, 300.0, 320], [0, 0, 1]])
HEIGHT = 4.0


def loop_course(lap=64, per_step=32, laps=1.25, seed=0):
    """A circular course of `lap` steps flown `laps` times over lap * per_step landmarks.  Returns dict(rows [M, 32] the landmarks'
    descriptor rows, xyz [M, 3]; frames: a list of dict(landmarks [n] indices, rows [n, 32] as observed, xy [n, 2] float32 pixels,
    R, t world -> camera)).  Deterministic in its arguments."""
    rng = np.random.default_rng(seed)
    M = lap * per_step
    radius = lap / (2 * np.pi)                            # a step is one unit of arc
    rows = rng.integers(0, 256, (M, 32), dtype=np.uint8)
    along = (np.arange(M) + 0.5) / per_step               # position along the course, in steps
    th = 2 * np.pi * along / lap
    r = radius + rng.uniform(-1, 1, M)
    xyz = np.stack([r * np.cos(th), r * np.sin(th), rng.uniform(-0.5, 0.5, M)], axis=1)
    frames = []
    for f in range(int(round(lap * laps))):
        p = f % lap + SIDE_STEP * (f // lap)
        d = np.abs(along - p)
        seen = np.flatnonzero(np.minimum(d, lap - d) < VIEW / 2)
        a = 2 * np.pi * p / lap
        R = np.array([[-np.sin(a), np.cos(a), 0], [np.cos(a), np.sin(a), 0], [0, 0, -1.0]])   # x along the track, looking down
        c = np.array([radius * np.cos(a), radius * np.sin(a), HEIGHT])
        t = -R @ c
        Xc = xyz[seen] @ R.T + t
        xy = ((Xc / Xc[:, 2:]) @ CAMERA.T)[:, :2].astype(np.float32)
        obs = rows[seen].copy()
        for k in range(len(seen)):
            for b in rng.choice(256, int(rng.integers(0, MAX_FLIPS + 1)), replace=False):
                obs[k, b // 8] ^= np.uint8(1 << (b % 8))
        frames.append(dict(landmarks=seen, rows=obs, xy=xy, R=R, t=t))
    return dict(rows=rows, xyz=xyz, frames=frames, lap=lap)


def true_revisits(course, min_gap, overlap=0.6):
    """{frame: [frames at least min_gap away that share at least `overlap` of the larger landmark set]}, ground truth"""
    fr = course["frames"]
    sets = [set(f["landmarks"].tolist()) for f in fr]
    out = {}
    for i in range(len(fr)):
        out[i] = [j for j in range(len(fr)) if abs(i - j) >= min_gap and len(sets[i] & sets[j]) >= overlap * max(len(sets[i]), len(sets[j]))]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lap", type=int, default=64)
    ap.add_argument("--per-step", type=int, default=32)
    ap.add_argument("--words", type=int, default=1024)
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
    from visual_odometry_amd import frontend as F
    course = loop_course(a.lap, a.per_step, seed=a.seed)
    frames = course["frames"]
    n = len(frames)
    per_frame = max(len(f["rows"]) for f in frames)
    min_gap = a.lap // 2
    min_shared = int(0.5 * VIEW * a.per_step)             # half a view: between a neighbouring place (2/3) and the next but one (1/4)
    truth = true_revisits(course, min_gap)

    fe = F.FrontEnd(64, 64, max_frames=n, max_pairs=1, nfeatures=max(304, per_frame), nlevels=1)
    assert fe.kp_cap >= per_frame
    for slot, f in enumerate(frames):
        fe.set_orb_rows(slot, f["rows"], f["xy"])
    rounds = fe.train_vocabulary(range(a.lap), K=a.words)
    fe.places_open(n)
    ids = np.arange(n)
    fe.places_add(range(n), ids)
    res = fe.places_query(top_k=2, min_gap=min_gap, min_shared=min_shared)
    cands = F.loop_candidates(res, ids)
    print(f"{n} frames, {per_frame} rows a frame at most, {a.words} words after {rounds} updates; min_gap {min_gap}, min_shared {min_shared}")
    print("frame  found (shared)                     true revisits")
    wrong = missed = 0
    for i in range(n):
        found = [(int(res["id"][i, k]), int(res["shared"][i, k])) for k in range(res["entry"].shape[1]) if res["entry"][i, k] >= 0]
        if not found and not truth[i]:
            continue
        wrong += sum(j not in truth[i] for j, _ in found)
        missed += bool(truth[i]) and not found
        print(f"{i:5d}  {', '.join(f'{j} ({s})' for j, s in found):34s} {truth[i]}")
    print(f"{len(cands)} candidate pairs; {wrong} reported frames are no true revisit, {missed} revisiting frames found nothing")
    if not cands:
        return
    # the best candidate, where it goes next: the newer frame placed in a map of the older frame's landmarks
    i, j, s = max(cands, key=lambda c: c[2])
    new, old = max(i, j), min(i, j)
    fo = frames[old]
    fe.stage_map(fo["rows"], course["xyz"][fo["landmarks"]])
    out = fe.relocalize([new], CAMERA)
    P = out["poses"][0]
    fn = frames[new]
    dR = np.degrees(np.arccos(np.clip((np.trace(P[:, :3] @ fn["R"].T) - 1) / 2, -1, 1)))
    dc = np.linalg.norm(-P[:, :3].T @ P[:, 3] + fn["R"].T @ fn["t"])
    print(f"best pair ({old}, {new}), shared {s}: relocalize status {int(out['status'][0])}, {int(out['n_match'][0])} matches, "
          f"{int(out['n_inl'][0])} inliers; rotation off by {dR:.3f} deg, camera centre by {dc:.4f} steps")


if __name__ == "__main__":
    main()
