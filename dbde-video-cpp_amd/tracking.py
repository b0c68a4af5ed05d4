"""Following objects through a stream with Codec.patch_moments: centres -> origins -> moments ->
centres, one frame at a time, everything on the device.

follow() is the loop a tracker of worms, cells, beads or stars runs: a small window per object, placed around the
object's last known centre, reduced to a mass and a centroid straight from the compressed bytes; the centroid is the
next frame's centre.  Out of scope here: a file-level driver (read a .dbde file batch by batch; dbde_video_cpp_amd.
streaming has the reader), threshold maps (a background image per sensor pixel instead of the two scalars), and
sub-pixel windows (origins are whole pixels: origins_from_centres rounds).
"""
import torch

from . import PatchMoments


def follow(codec, stream, stream_offset, stream_bytes, offsets, W, H, n, centres0, pw, ph, lo, hi, weight="above",
           edge="fill", bits=8):
    """Follows K objects through n frames (frame f at stream.data_ptr()+stream_offset+offsets[f]).

    centres0: (K, 2) (x, y) centres for frame 0, anything torch.as_tensor takes.  Frame f's patch origins are
    origins_from_centres of frame f-1's centres (centres0 for f = 0); its centres are the centroids
    PatchMoments.centroid() gives for those patches.  An object with S = 0 in a frame (nothing selected, the patch
    outside the frame, or the frame rejected) keeps its last centre.  One patch_moments call per frame on the codec's
    stream; nothing is copied to the host, and no tensor is built from host data inside the loop, so the host never waits
    for the device there (with centres0 already a device tensor, nowhere in the call).  bits: 8 for DBDE, 16 for DBDE16 streams.

    Returns (centres float64 (n, K, 2), PatchMoments with moments (n, K, 8), bbox (n, K, 4) and used (n, K, 2)).  The
    moments, box and used origins of a rejected frame are 0, (pw, ph, -1, -1) and the origins asked for."""
    if bits not in (8, 16):
        raise ValueError("bits must be 8 or 16")
    call = codec.patch_moments if bits == 8 else codec.patch_moments16
    with torch.cuda.stream(codec.stream):
        c = torch.as_tensor(centres0, dtype=torch.float64, device=codec.device)
        if c.dim() != 2 or c.shape[1] != 2:
            raise ValueError("centres0 must have shape (K, 2)")
        K = int(c.shape[0])
        # Every tensor is made on the device and filled from Python scalars: a tensor built from host data (a list, a numpy
        # array) is a pageable copy that waits for the stream.  With centres0 already on the device, follow() never waits.
        dev = codec.device
        centres = torch.empty((n, K, 2), dtype=torch.float64, device=dev)
        moments = torch.zeros((n, K, 8), dtype=torch.int64, device=dev)
        bbox = torch.full((n, K, 4), -1, dtype=torch.int32, device=dev)
        bbox[..., 0] = pw
        bbox[..., 1] = ph
        used = torch.empty((n, K, 2), dtype=torch.int32, device=dev)
        results = torch.empty((n, 4), dtype=torch.int64, device=dev)
        half = torch.empty(2, dtype=torch.int64, device=dev)   # origins_from_centres' (pw // 2, ph // 2), made once
        half[:1].fill_(pw // 2)   # (fill_, not half[0] = ...: an indexed assignment of a scalar goes through a host tensor)
        half[1:].fill_(ph // 2)
        for f in range(n):
            # origins_from_centres(c, pw, ph), restated with the prebuilt half sizes: floor(c + 0.5) - p // 2, clamped to int32
            org = (torch.floor(c + 0.5).to(torch.int64) - half).clamp(-2 ** 31, 2 ** 31 - 1).to(torch.int32).reshape(1, K, 2)
            used[f] = org[0]   # (a rejected frame leaves the entry untouched)
            pm, _ = call(stream, stream_offset, stream_bytes, offsets[f:f + 1], W, H, 1, pw, ph, org, lo, hi,
                         weight=weight, edge=edge, out=moments[f:f + 1], bbox=bbox[f:f + 1], used=used[f:f + 1],
                         results=results[f:f + 1])
            got = pm.centroid()[0]
            c = torch.where(torch.isnan(got), c, got)
            centres[f] = c
    return centres, PatchMoments(moments, bbox, used, pw, ph)
