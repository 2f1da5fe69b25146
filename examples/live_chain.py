#!/usr/bin/env python3
"""The reference's live configuration, files in -> trajectory out, as one resident pipeline on an MI355X (no map optimisation, no viewer):

    cv2.imread(4K .jpg) -> cv2.resize(x 0.3) -> cv2.SIFT_create().detectAndCompute -> BFMatcher(NORM_L2, crossCheck) -> findEssentialMat
    -> recoverPose -> triangulatePoints                     (src/visual_slam.py:346-352, :17, :19, :294-298)
    -> update_feature_mapper / estimate_current_camera_position (solvePnPRansac) / add_information_to_map   (:183-266, :153-180)

Only the compressed file bytes cross PCIe; every stage after that reads what the previous one left in HBM.
    python examples/live_chain.py [--frames 8] [--width 3840 --height 2160 --scale 0.3] [--detector sift|orb] [--step 4.0] [--restart] [--stream N] [--dist k1,k2,p1,p2[,k3]] [--join MAX_ERROR [--blank F]]
--restart: afterwards the complete map step (bundle adjustment, filter, camera limit) on the same resident pairs with restart=True — a lost frame
starts a new map instead of ending the chain — and one track per segment, each in its own gauge.
--stream N: the same files once more in chunks of N pairs through slam_stream on a front end with only N + 1 frame slots — the map stays on the
device between the chunks, every chunk's files are decoded into the slots the chunk before freed — and the track, which is the track of one
slam_chain call on all the files.
--stream N --restart together: the chunks go through slam_stream_restart instead — a lost frame starts a new map in whichever chunk it falls,
and a chunk that ends lost is continued — and one track per segment is printed from the joined calls (join_stream, split_segments); they are the
segments of slam_chain(restart=True) on all the files.
--dist k1,k2,p1,p2[,k3]: a camera with a real lens — after each detection the keypoints are undistorted on the device (FrontEnd.undistort,
cv2.undistortPoints' arithmetic) and everything after runs on ideal pixels.  (The synthetic frames here come from a pinhole, so the option shows
the call in place, not a better track.)  Without it the output is what it was.
--join MAX_ERROR [--blank F]: the segments of slam_chain(restart=True) in ONE gauge.  While the frames are resident every segment's pairs run
once more as a sequence of slam_chains and its map is saved (map_from_slam + map_rows: points and their descriptor rows); every later map is
aligned to the one before it by those rows (stage_map + align_maps: the similarity between the two gauges, MAX_ERROR in the earlier map's
units, its first pair's baseline); join_segments composes the similarities and one track is printed.  --blank F replaces file F by a gray
frame, so that there is a loss to join across."""
import argparse
import io
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from visual_odometry_amd import ingest, synth  # noqa: E402
from visual_odometry_amd.frontend import FrontEnd, join_segments, join_stream, split_segments  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--width", type=int, default=3840); ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--scale", type=float, default=0.3, help="the reference's scale_percent / 100")
    ap.add_argument("--detector", choices=["sift", "orb"], default="sift")
    ap.add_argument("--step", type=float, default=4.0, help="flight distance per frame (the camera is 30 units above the ground)")
    ap.add_argument("--restart", action="store_true", help="also run slam_chain(restart=True) and print one track per segment")
    ap.add_argument("--stream", type=int, default=0, metavar="N", help="also walk the files in chunks of N pairs through slam_stream (N + 1 frame slots)")
    ap.add_argument("--dist", type=lambda s: [float(v) for v in s.split(",")], default=None, metavar="k1,k2,p1,p2[,k3]",
                    help="lens distortion coefficients: undistort the keypoints on the device after each detection (FrontEnd.undistort)")
    ap.add_argument("--join", type=float, default=0.0, metavar="MAX_ERROR", help="join the restart segments into one gauge by their maps' descriptors (align_maps)")
    ap.add_argument("--blank", type=int, default=-1, metavar="F", help="replace file F by a gray frame: a lost frame")
    a = ap.parse_args()
    if a.dist is not None and len(a.dist) not in (4, 5):
        ap.error("--dist takes 4 or 5 comma-separated coefficients")
    from PIL import Image
    n = a.frames
    dw, dh = int(a.width * a.scale), int(a.height * a.scale)
    # a seeded synthetic flight rendered at the working size, blown up to "camera" files (there is no footage in the repository)
    seq = synth.sequence(n, dw, dh, step=a.step)
    files = []
    for f, g in enumerate(seq["frames"]):
        if f == a.blank:
            g = np.full_like(g, 127)
        b = io.BytesIO()
        Image.fromarray(np.stack([g, g, g], -1)).resize((a.width, a.height), Image.BICUBIC).save(b, "JPEG", quality=92)
        files.append(b.getvalue())
    K = seq["K"]
    fe = FrontEnd(dh, dw, max_frames=n, max_pairs=n - 1, detector=a.detector, **({} if a.detector == "sift" else {"nfeatures": 2000}))
    pairs = [[k, k + 1] for k in range(n - 1)]
    packed = ingest.PackedFiles(files)                          # page-locked: the upload is one DMA transfer
    t0 = time.perf_counter()
    fe.ingest_jpeg(packed)                                      # decode + resize + gray on the device
    fe.detect(0, n)
    if a.dist is not None:
        fe.undistort(0, n, K, a.dist)                           # K is the matrix of the resized frames; the coefficients survive a resize
    res, _ = fe.run_pairs(pairs, K, want_points=True)
    out = fe.localize_chain(n - 1, K)                           # tracks -> solvePnPRansac -> cameras -> new map points
    dt = time.perf_counter() - t0
    print(f"{n} files {a.width}x{a.height} ({sum(map(len, files)) / n / 1024:.0f} KiB each) -> {dw}x{dh} -> {a.detector.upper()} -> {n - 1} pairs -> chain: {1e3 * dt:.1f} ms")
    centres = np.array([-P[:, :3].T @ P[:, 3] for P in out["poses"]])
    for k in range(n - 1):
        print(f"pair {k}->{k + 1}: keypoints {res['n_kp1'][k]}/{res['n_kp2'][k]} matches {res['n_match'][k]} E-inliers {res['n_inl'][k]} | "
              f"PnP {out['n_inl'][k]}/{out['n_corr'][k]} status {out['status'][k]} map {out['n_map'][k]} | camera {k + 1} at {np.round(centres[k + 1], 2)}")
    if a.restart:
        out = fe.slam_chain(n - 1, K, restart=True)             # the map step; tracking lost -> a new map from the next usable pair
        print(f"slam_chain(restart=True): status {out['status'].tolist()} segment {out['segment'].tolist()} cause {out['cause'].tolist()}")
        for i, sg in enumerate(out["segments"]):
            track = np.array([-P[:, :3].T @ P[:, 3] for P in sg["poses"]])
            print(f"segment {i}: frames {sg['first_pair']}..{sg['first_pair'] + sg['n_pairs']}, camera centres in its own gauge:")
            print(np.round(track, 2))
    if a.join > 0:
        segs = fe.slam_chain(n - 1, K, restart=True)["segments"]
        seg_pairs = [[[sg["first_pair"] + j, sg["first_pair"] + j + 1] for j in range(sg["n_pairs"])] for sg in segs]
        fe.run_pairs([p for sp in seg_pairs for p in sp], K, want_points=True)
        chains = fe.slam_chains([len(sp) for sp in seg_pairs], K)  # every segment as a sequence of its own: its track and its map
        maps = []
        for k in range(len(segs)):
            fe.map_from_slam(seq=k)                             # on the device, while the segment's frames are in their slots
            maps.append(fe.map_rows())                          # (rows, points): what survives the frames
        sims = []
        for k in range(1, len(segs)):
            fe.stage_map(*maps[k - 1])
            r = fe.align_maps(*maps[k], max_error=a.join)       # segment k's gauge -> segment k - 1's
            print(f"segments {k - 1} <- {k}: maps of {len(maps[k - 1][0])} and {len(maps[k][0])} points, {r['n_match'][0]} matches, {r['n_inl'][0]} inliers, "
                  f"status {r['status'][0]}, scale {r['scale'][0]:.4f}")
            sims.append(None if r["status"][0] else (r["scale"][0], r["R"][0], r["t"][0]))
        tracks = [dict(first_pair=sg["first_pair"], n_pairs=sg["n_pairs"], poses_pnp=c["poses_pnp"], poses=c["poses"]) for sg, c in zip(segs, chains)]
        joined, loose = join_segments(tracks, sims)
        print(f"one track in segment 0's gauge ({len(joined)} of {len(segs)} segments joined; not connected: {loose}):")
        for sg in joined:
            track = np.array([-P[:, :3].T @ P[:, 3] for P in sg["poses"]])
            print(f"frames {sg['first_pair']}..{sg['first_pair'] + sg['n_pairs']} (scale {sg['sim'][0]:.4f}):")
            print(np.round(track, 2))
    if a.stream > 0:
        whole = fe.slam_chain(n - 1, K, restart=a.restart)      # the yardstick: one call, every frame resident
        N = min(a.stream, n - 1)
        st = FrontEnd(dh, dw, max_frames=N + 1, max_pairs=N, detector=a.detector, **({} if a.detector == "sift" else {"nfeatures": 2000}))
        slots, last, outs = list(range(N + 1)), np.zeros((n, 3, 4)), []
        call, name = (st.slam_stream_restart, "slam_stream_restart") if a.restart else (st.slam_stream, "slam_stream")
        for c, first in enumerate(range(0, n - 1, N)):          # the chunk's pairs: first .. first + b - 1
            b = min(N, n - 1 - first)
            new = slots[:b + 1] if c == 0 else slots[1:b + 1]
            for slot, f in zip(new, range(first + (c > 0), first + b + 1)):
                st.ingest_jpeg([files[f]], first_slot=slot); st.detect(slot, 1)
                if a.dist is not None:
                    st.undistort(slot, 1, K, a.dist)            # the chunk's new frames only: the anchor slot was undistorted in its own chunk
            st.run_pairs([[slots[j], slots[j + 1]] for j in range(b)], K, want_points=True)
            out = call(b, K, resume=c > 0, total_pairs=n - 1)
            outs.append(out)
            for f, T in zip(out["carried_frame"], out["carried_poses"]):
                last[f] = T                                     # a camera of an earlier chunk, as the map last held it in this call
            last[first:first + b + 1] = out["poses"]
            print(f"{name} chunk {c}: frames {first}..{first + b} in slots {slots[:b + 1]}, status {out['status'].tolist()}, map {out['n_cam'][-1]} cameras "
                  f"{out['n_pts'][-1]} points, carried {out['carried_frame'].tolist()}")
            slots = [slots[b]] + slots[:b] + slots[b + 1:]      # the chunk's last frame stays where it is
        if not a.restart:
            print(f"slam_stream in chunks of {N}: the track {'equals' if np.array_equal(last, whole['poses']) else 'DIFFERS from'} slam_chain's on all {n} files; camera centres:")
            print(np.round(np.array([-P[:, :3].T @ P[:, 3] for P in last]), 2))
        else:
            j = join_stream(outs)                               # the whole flight's arrays from the calls' rows, seg_poses rows and carried rows
            segs = split_segments(j["segment"], j["poses_pnp"], j["poses"], j["seg_poses_pnp"], j["seg_poses"])
            same = len(segs) == len(whole["segments"]) and all(np.array_equal(x["poses"], y["poses"]) for x, y in zip(segs, whole["segments"]))
            print(f"slam_stream_restart in chunks of {N}: segment {j['segment'].tolist()} cause {j['cause'].tolist()}; the segments "
                  f"{'equal' if same else 'DIFFER from'} slam_chain(restart=True)'s on all {n} files")
            for i, sg in enumerate(segs):
                print(f"segment {i}: frames {sg['first_pair']}..{sg['first_pair'] + sg['n_pairs']}, camera centres in its own gauge:")
                print(np.round(np.array([-P[:, :3].T @ P[:, 3] for P in sg["poses"]]), 2))


if __name__ == "__main__":
    main()
