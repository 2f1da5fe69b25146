#!/usr/bin/env python3
"""A loop closed against the map a stream built: a flight that goes out and comes back, streamed in chunks with slot reuse.

    python examples/loop_flight.py [--out 8] [--chunk 4] [--window 1] [--max-cameras 18] [--width 640] [--height 480] [--nfeatures 1000] [--ratio R] [--guided R]

The flight is synthetic and uses no files: frames 0 .. n of synth.sequence, then n - 1 .. 0 again, so the last frames see the ground
of the first.  It is walked by slam_stream in chunks of --chunk pairs on a FrontEnd with only chunk + 2 frame slots: every chunk's
frames go into the slots the chunk before freed, and when the flight is back at its start the frames of its beginning have long left
the device.  The stream runs with a descriptor store (stream_rows) and an archive of evicted points (stream_archive), so what it
has mapped can still be matched against.

Every frame becomes an entry of the keyframe index while it is resident (train_vocabulary on the first chunk, places_add); at the
end places_query -> loop_candidates names pairs (old, new) of frames that see the same place.  For the best candidate whose `new`
frame is still in a slot, map_from_stream_archive(old - w, old + w + 1) stages the points owned by the frames around `old` — the live
ones from the store, the ones the camera limit has removed from the archive; their slots are gone — and relocalize places `new`
among them by its descriptors alone.  Printed: that pose against the pose the
stream itself gave `new` through its chain of pairs (--ratio R: matched by Lowe's ratio rule, knnMatch(k=2) and
`m.distance < R * n.distance`, instead of the cross-check); the difference is the drift the flight accumulated between the two visits.
The loop_edge the pose graph would take for (old, new) is built from the two (optimize_pose_graph, examples/close_loop.py).
--guided R: before the edge is built, the wider window old - 3 w - 2 .. old + 3 w + 2 is staged and relocalize_guided matches its
points by projection under the pose just found, within R pixels of each projection; matches and inliers before and after are printed,
and the edge is built from the refined pose.

The stream's map is its LIVE map: a point the camera limit has removed (--max-cameras, the reference's 18 by default) is gone from
it.  With the default flight of 17 frames nothing is evicted; fly further out (--out 20) or lower --max-cameras (--max-cameras 4) and
the points around the flight's start are staged from the archive."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", type=int, default=8, help="frames flown out before turning back")
    ap.add_argument("--chunk", type=int, default=4)
    ap.add_argument("--window", type=int, default=1)
    ap.add_argument("--max-cameras", type=int, default=18, help="cameras the map keeps (limit_number_of_camera_in_map)")
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--nfeatures", type=int, default=1000)
    ap.add_argument("--words", type=int, default=256)
    ap.add_argument("--ratio", type=float, default=None, help="relocalize by the ratio rule with this ratio instead of the cross-check")
    ap.add_argument("--guided", type=float, default=None, metavar="R",
                    help="refine the pose by projection matching within R pixels against a wider window of the map")
    a = ap.parse_args()
    from visual_odometry_amd import frontend as F
    from visual_odometry_amd import synth
    seq = synth.sequence(a.out + 1, a.width, a.height, step=4.0, cache_dir="/tmp")
    image = list(range(a.out + 1)) + list(range(a.out - 1, -1, -1))      # the image every frame of the flight shows
    n, pairs, K = len(image), len(image) - 1, seq["K"]
    n_slots = a.chunk + 2
    fe = F.FrontEnd(a.height, a.width, max_frames=n_slots, max_pairs=a.chunk, nfeatures=a.nfeatures)
    fe.stream_rows(-1)                                                    # a row for every feature the stream can hold: nothing is dropped
    fe.stream_archive(-1)                                                 # ... and an entry: every point the camera limit removes is kept

    free, slot_of, poses, at = list(range(n_slots)), {}, np.zeros((n, 3, 4)), 0
    while at < pairs:
        b = min(a.chunk, pairs - at)
        new = list(range(at + (at > 0), at + b + 1))                      # the stream's last frame stays in its slot
        for f in new:
            slot_of[f] = free.pop(0)
            fe.upload(seq["frames"][image[f]][None], first_slot=slot_of[f]); fe.detect(slot_of[f], 1)
        if at == 0:
            fe.train_vocabulary([slot_of[f] for f in new], K=a.words)
            fe.places_open(n)                                             # (a new vocabulary closes an open index: train first)
        fe.places_add([slot_of[f] for f in new], new)
        fe.run_pairs([[slot_of[at + j], slot_of[at + j + 1]] for j in range(b)], K, want_points=True)
        out = fe.slam_stream(b, K, resume=at > 0, total_pairs=pairs, max_cameras=a.max_cameras)
        if (out["status"] != 0).any():
            raise SystemExit(f"the stream lost track in the chunk at pair {at}: status {out['status'].tolist()}")
        for f, T in zip(out["carried_frame"], out["carried_poses"]):      # every frame's pose as the map last held it
            poses[int(f)] = T
        poses[at:at + b + 1] = out["poses"]
        for f in range(at, at + b if at + b < pairs else at):             # every frame but the chunk's last gives its slot back; the last chunk stays
            free.append(slot_of.pop(f))
        free.sort()
        at += b
    info, arc, m = fe.stream_rows_info(), fe.stream_archive_info(), fe.slam_map(0)
    print(f"{n} frames ({a.out} out, {a.out} back) in chunks of {a.chunk} pairs on {n_slots} slots; live map {len(m['points'])} points of "
          f"{len(m['cam_frame'])} cameras (at most {a.max_cameras}); store: {info['stored']} rows of {info['capacity']}, {info['dropped']} dropped; "
          f"archive: {arc['stored']} evicted points of {arc['capacity']}, {arc['dropped']} dropped")

    ids = np.arange(n)
    res = fe.places_query(top_k=2, min_gap=a.chunk + 2)
    cands = [(min(i, j), max(i, j), s) for i, j, s in F.loop_candidates(res, ids)]
    resident = [c for c in cands if c[1] in slot_of]
    print(f"{len(cands)} loop candidates, {len(resident)} with the newer frame still in a slot (frames {sorted(slot_of)})")
    if not resident:
        return
    old, new, shared = max(resident, key=lambda c: c[2])
    first, end = max(old - a.window, 0), old + a.window + 1
    staged = fe.map_from_stream_archive(first, end)
    print(f"best candidate ({old}, {new}), {shared} shared words (images {image[old]} and {image[new]}); "
          f"map_from_stream_archive({first}, {end}): {staged['n']} points, {staged['n'] - staged['n_archived']} live and "
          f"{staged['n_archived']} archived, {staged['without_row']} without a row")
    r = fe.relocalize([slot_of[new]], K) if a.ratio is None else fe.relocalize([slot_of[new]], K, match="ratio", ratio=a.ratio)
    if r["status"][0] != 0:
        print(f"relocalize: status {int(r['status'][0])} with {int(r['n_match'][0])} matches")
        return
    P, Q = r["poses"][0], poses[new]                                      # by the old frames' points; by the stream's own chain
    print(f"relocalize: {int(r['n_match'][0])} matches, {int(r['n_inl'][0])} inliers")
    if a.guided is not None:
        wide = (max(old - 3 * a.window - 2, 0), old + 3 * a.window + 3)
        staged = fe.map_from_stream_archive(*wide)
        g = fe.relocalize_guided([slot_of[new]], K, r["poses"], a.guided)
        print(f"guided, {a.guided:g} px under that pose against map_from_stream_archive{wide} ({staged['n']} points, {int(g['n_seen'][0])} with a keypoint "
              f"in their window): {int(g['n_match'][0])} matches, {int(g['n_inl'][0])} inliers (before: {int(r['n_match'][0])}, {int(r['n_inl'][0])})")
        if g["status"][0] != 0:
            print(f"guided: status {int(g['status'][0])}: the descriptor-only pose is kept")
        elif g["n_inl"][0] <= r["n_inl"][0]:
            print("guided: no more inliers than before (the wider window adds few points this frame sees, or the radius is too small "
                  "for the pose's error): the descriptor-only pose is kept")
        else:
            P = g["poses"][0]
    dR = np.degrees(np.arccos(np.clip((np.trace(P[:, :3] @ Q[:, :3].T) - 1) / 2, -1, 1)))
    cP, cQ = -P[:, :3].T @ P[:, 3], -Q[:, :3].T @ Q[:, 3]
    base = np.linalg.norm(-poses[1][:, :3].T @ poses[1][:, 3])            # the gauge's unit: the first pair's baseline
    print(f"frame {new} by the map around frame {old} against the stream's own pose: rotation {dR:.4f} deg, camera centre "
          f"{np.linalg.norm(cP - cQ):.5f} ({np.linalg.norm(cP - cQ) / max(base, 1e-12):.4f} baselines): the drift between the two visits")
    V = F.track_vertices(poses)
    edge = F.loop_edge(V[old], F.track_vertices(P[None])[0])
    print(f"loop edge ({old}, {new}) for optimize_pose_graph: scale {edge[0]:.4f}, t {np.round(edge[10:], 5).tolist()}")


if __name__ == "__main__":
    main()
