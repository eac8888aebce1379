"""Do two builds of the library enqueue the same kernels?  A short fixed workload for `rocprofv3 --kernel-trace`, and the listing
of a trace: per hardware queue (numbered by first use) the kernels in dispatch order, each with its grid.

usage: rocprofv3 --kernel-trace -d <dir> -o trace -- python3 tools/enqueue_trace.py run      (FT_LIB selects the build)
       python3 tools/enqueue_trace.py list <dir>  >  listing.txt                              (diff the listings of two builds)

The workload walks the paths of the front end's host code: a wide extract (device octree, sub-batches), a small extract twice
(graph capture, then replay), the same three for the stereo front end (wide, paired capture, replay), and a wide stereo batch
on the host-octree pipeline."""
import glob
import os
import sqlite3
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def run():
    from fasttrack_amd import orb, synth
    w, h, nf = 640, 480, 1000
    intr = synth.intrinsics(w, h)
    pairs = [synth.make_stereo_pair(w, h, 40 + b) for b in range(32)]
    left, right = [p[0] for p in pairs], [p[1] for p in pairs]
    ctx = orb.Context(0)
    ex32 = orb.ORBextractor(ctx, nf, 1.2, 8, 20, 7, w, h, max_batch=32)
    ex32.extract_batch(left)
    ex2 = orb.ORBextractor(ctx, nf, 1.2, 8, 20, 7, w, h, max_batch=2)
    ex2.extract_batch(left[:2])
    ex2.extract_batch(left[2:4])
    fe32 = orb.StereoFrontend(ctx, nf, 1.2, 8, 20, 7, w, h, 32, intr["mbf"], intr["mb"])
    fe32.process(left, right)
    fe2 = orb.StereoFrontend(ctx, nf, 1.2, 8, 20, 7, w, h, 2, intr["mbf"], intr["mb"])
    fe2.process(left[:2], right[:2])
    fe2.process(left[2:4], right[2:4])
    with ctx.options(device_octree=0):
        feh = orb.StereoFrontend(ctx, nf, 1.2, 8, 20, 7, w, h, 32, intr["mbf"], intr["mb"])
    feh.process(left, right)
    for name in ("extract.graph_captures", "stereo.graph_captures", "stereo.graph_launch", "extract.device_octree_batches",
                 "stereo.device_octree_batches", "stereo.octree(host,both)"):
        try:
            print(name, ctx.get_stat(name)[1])
        except Exception:
            print(name, 0)


def listing(root):
    rows = []
    for f in sorted(glob.glob(os.path.join(root, "**", "*.db"), recursive=True)):
        db = sqlite3.connect(f)
        rows += list(db.execute("select queue_id, dispatch_id, name, grid_x, grid_y, grid_z, workgroup_x from kernels"))
    rows.sort(key=lambda r: r[1])
    queues = {}
    for q, _, name, gx, gy, gz, wx in rows:
        name = name.replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0]
        queues.setdefault(q, []).append(f"{name} grid {gx}x{gy}x{gz} wg {wx}")
    for k, q in enumerate(queues):  # (dicts keep insertion order: queues in the order of their first dispatch)
        print(f"== queue {k}: {len(queues[q])} kernels")
        print("\n".join(queues[q]))


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "list":
        listing(sys.argv[2])
    else:
        run()
