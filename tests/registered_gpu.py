"""What the tests of the registered projections share (test infrastructure, like lag_gpu.py; not a test module): the
cap that keeps a case from passing with the origins ignored, transposed or off by one, and the one check every GPU case
runs -- the call against tests/registered_ref.py, by equality.  The streams are lag_gpu's (crafted on the host from a
seed, so that the CPU test can judge their content before any GPU run)."""
import numpy as np

import lag_gpu as lg
import registered_ref as rr

SENT = -77          # origins_used rows of rejected frames keep it


def images_of(spec):
    return lg.host_images(*spec)


def cap(images, spec, rw, rh, origins, mask):
    """The expected planes, after the cap.  With the clamped origins o (what the call must use):
      (a) every origin replaced by frame 0's;  (b) x and y swapped;  (c) every origin + 1 in x, and + 1 in y
    -- each only where the changed origins are valid (inside [0, W - rw] x [0, H - rh], so that the clamp does not undo
    the change) and differ from o.  On noise every requested plane must differ from each of them; on other content at
    least one plane must differ under (a).  A window that has only one possible origin (the whole frame) and a stream
    without an accepted frame have nothing to tell apart."""
    kind, _, W, H, n, bits, _ = spec
    want = rr.registered(images, origins, rw, rh, bits)
    names = rr.names_of(mask)
    live = [f for f in range(n) if images[f] is not None]
    if not live or (rw == W and rh == H):
        return want
    o = rr.clamp(origins, W, H, rw, rh)

    def valid(v):
        return (v[:, 0] >= 0).all() and (v[:, 0] <= W - rw).all() and (v[:, 1] >= 0).all() and (v[:, 1] <= H - rh).all()

    variants = {"a": np.repeat(o[live[:1]], n, 0), "b": o[:, ::-1], "cx": o + (1, 0), "cy": o + (0, 1)}
    for tag, v in variants.items():
        if not valid(v[live]) or np.array_equal(v[live], o[live]):
            assert tag != "a", "every accepted frame has the same origin: the case shows nothing"
            continue
        wrong = rr.registered(images, v, rw, rh, bits)
        differs = [k for k in names if not np.array_equal(want[k], wrong[k])]
        if kind == "noise":
            assert differs == list(names), (tag, "planes that do not tell", set(names) - set(differs))
        elif tag == "a":
            assert differs, "no plane tells the origins from frame 0's"
    return want


def planes(out):
    """Projection's requested planes on the host: max / min in the pixel type, the sums as the U64 bits."""
    got = {}
    for k in rr.STATS:
        t = getattr(out, k)
        if t is None:
            continue
        t = t.cpu().numpy()
        got[k] = t.view(np.uint64) if k in ("sum", "sumsq") else t.view(np.uint16) if t.dtype == np.int16 else t
    return got


def compare(out, want, names, what):
    got = planes(out)
    assert tuple(got) == tuple(names), (what, tuple(got), names)
    for k in names:
        assert got[k].shape == want[k].shape and got[k].dtype == want[k].dtype, (what, k, got[k].dtype, got[k].shape)
        if not np.array_equal(got[k], want[k]):
            bad = tuple(np.argwhere(got[k] != want[k])[0])
            raise AssertionError(f"{what}: {k} differs at {bad}: {got[k][bad]} != {want[k][bad]}; "
                                 f"{int((got[k] != want[k]).sum())} of {got[k].size} elements")
    assert int(out.count.item()) == want["count"], (what, "count")


def device_origins(origins):
    import torch
    return torch.from_numpy(np.asarray(origins, np.int64).astype(np.int32)).cuda().contiguous()


def call_of(codec, bits):
    return codec.project_registered if bits == 8 else codec.project_registered16


def check(codec, case, use_cap=True, **kw):
    """One call of the case against registered_ref: the planes, the count and origins_used.  Returns (out, results)."""
    import torch
    name, spec, rw, rh, origins, mask = case
    bits = spec[5]
    s = lg.stream(*spec)
    want = cap(s.images, spec, rw, rh, origins, mask) if use_cap else rr.registered(s.images, origins, rw, rh, bits)
    names = rr.names_of(mask)
    used = torch.full((s.n, 2), SENT, dtype=torch.int32, device="cuda")
    out, res = call_of(codec, bits)(s.buf, s.lead, s.total, s.offs, s.W, s.H, s.n, rw, rh, device_origins(origins),
                                    stats=names, origins_used=used, **kw)
    torch.cuda.synchronize()
    compare(out, want, names, f"{name} {s.W}x{s.H} n={s.n} {rw}x{rh} mask={mask} {bits}-bit")
    u = used.cpu().numpy()
    for f in range(s.n):
        assert tuple(u[f]) == want["used"].get(f, (SENT, SENT)), (name, f, "origins_used")
    return out, res


def run(codec, cases):
    for case in cases:
        check(codec, case)
