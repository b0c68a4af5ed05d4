"""One rank of the stand-in transport's own test (tests/test_fake_rccl.py), in host mode: plays a program of collective
steps the parent wrote, calling libdbde_fake_rccl.so through ctypes on numpy buffers, and saves what it received.
Needs numpy only -- neither the package nor a GPU.

    python host_rank.py <library> <program.json> <rank> <out.npz>

program.json: {"world", "id_file", "ranks": [[step, ...] per rank]}; a step is
    {"op": "allgather", "words": [..]}                      2 x U64 of this rank -> "out": 2 x world U64
    {"op": "broadcast", "root": r, "words": [..]}           in place, as dbde_scatter.cpp calls it
    {"op": "group", "ops": [[kind, peer, src, src_off, dst, dst_off, bytes], ..]}
                                                            kind "send" | "recv"; src in "data" | "aux"; dst in "canvas" | "canvas2"
    {"op": "recv_alone", "peer": p, "bytes": n}             a receive nobody answers: reports the code, the text, the seconds
    {"op": "leave"}                                         exits without another call
Inputs are the parent's to know: data = rng(1000 + rank) bytes, aux = rng(2000 + rank) bytes, canvases 0xEE."""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

DATA_BYTES = 48 << 10
NCCL_UINT8, NCCL_UINT64 = 1, 5


def inputs(rank):
    return (np.random.default_rng(1000 + rank).integers(0, 256, DATA_BYTES, dtype=np.uint8),
            np.random.default_rng(2000 + rank).integers(0, 256, DATA_BYTES, dtype=np.uint8))


class UniqueId(C.Structure):
    _fields_ = [("internal", C.c_char * 128)]


def load(path):
    L = C.CDLL(path)
    vp, sz, i = C.c_void_p, C.c_size_t, C.c_int
    L.ncclGetUniqueId.argtypes = [C.POINTER(UniqueId)]
    L.ncclCommInitRank.argtypes = [C.POINTER(vp), i, UniqueId, i]
    L.ncclCommDestroy.argtypes = [vp]
    L.ncclAllGather.argtypes = [vp, vp, sz, i, vp, vp]
    L.ncclBroadcast.argtypes = [vp, vp, sz, i, i, vp, vp]
    L.ncclSend.argtypes = [vp, sz, i, i, vp, vp]
    L.ncclRecv.argtypes = [vp, sz, i, i, vp, vp]
    L.ncclGetErrorString.restype = C.c_char_p
    L.ncclGetErrorString.argtypes = [i]
    L.ncclGetVersion.argtypes = [C.POINTER(i)]
    return L


def rendezvous(L, id_file, rank, deadline_s=30.0):
    """Rank 0 makes the id and publishes it (write, then rename); the others poll with a deadline."""
    uid = UniqueId()
    if rank == 0:
        assert L.ncclGetUniqueId(C.byref(uid)) == 0
        with open(id_file + ".tmp", "wb") as f:
            f.write(C.string_at(C.byref(uid), 128))
        os.rename(id_file + ".tmp", id_file)
        return uid
    t0 = time.monotonic()
    while not os.path.exists(id_file):
        if time.monotonic() - t0 > deadline_s:
            raise SystemExit(f"rank {rank}: no unique id after {deadline_s} s")
        time.sleep(0.005)
    with open(id_file, "rb") as f:
        C.memmove(C.byref(uid), f.read(), 128)
    return uid


def main():
    lib_path, program_path, rank, out_path = sys.argv[1], sys.argv[2], int(sys.argv[3]), sys.argv[4]
    with open(program_path) as f:
        program = json.load(f)
    world, steps = program["world"], program["ranks"][rank]
    L = load(lib_path)
    comm = C.c_void_p()
    rc = L.ncclCommInitRank(C.byref(comm), world, rendezvous(L, program["id_file"], rank), rank)
    if rc != 0:
        raise SystemExit(f"rank {rank}: ncclCommInitRank -> {rc}: {L.ncclGetErrorString(rc).decode()}")
    data, aux = inputs(rank)
    out = {}
    for k, step in enumerate(steps):
        if step["op"] == "leave":
            np.savez(out_path, **out)
            os._exit(0)
        if step["op"] == "allgather":
            mine = np.array(step["words"], np.uint64)
            got = np.full(2 * world, 0xEEEEEEEEEEEEEEEE, np.uint64)
            rc = L.ncclAllGather(mine.ctypes.data, got.ctypes.data, 2, NCCL_UINT64, comm, None)
            out[f"s{k}_out"] = got
        elif step["op"] == "broadcast":
            buf = np.array(step["words"], np.uint64)
            rc = L.ncclBroadcast(buf.ctypes.data, buf.ctypes.data, buf.size, NCCL_UINT64, step["root"], comm, None)
            out[f"s{k}_out"] = buf
        elif step["op"] == "group":
            src = {"data": data, "aux": aux}
            dst = {"canvas": np.full(DATA_BYTES, 0xEE, np.uint8), "canvas2": np.full(DATA_BYTES, 0xEE, np.uint8)}
            rcs = [L.ncclGroupStart()]
            for kind, peer, s, s_off, d, d_off, nbytes in step["ops"]:
                if kind == "send":
                    rcs.append(L.ncclSend(src[s].ctypes.data + s_off, nbytes, NCCL_UINT8, peer, comm, None))
                else:
                    rcs.append(L.ncclRecv(dst[d].ctypes.data + d_off, nbytes, NCCL_UINT8, peer, comm, None))
            rcs.append(L.ncclGroupEnd())
            rc = next((r for r in rcs if r), 0)
            out[f"s{k}_canvas"], out[f"s{k}_canvas2"] = dst["canvas"], dst["canvas2"]
        elif step["op"] == "recv_alone":
            buf = np.full(max(step["bytes"], 1), 0xEE, np.uint8)
            t0 = time.monotonic()
            rc = L.ncclRecv(buf.ctypes.data, step["bytes"], NCCL_UINT8, step["peer"], comm, None)
            out[f"s{k}_seconds"] = np.array(time.monotonic() - t0)
            out[f"s{k}_code"] = np.array(rc)
            out[f"s{k}_text"] = np.array(L.ncclGetErrorString(rc).decode())
            out[f"s{k}_out"] = buf
            rc = 0
        else:
            raise SystemExit(f"unknown step {step}")
        if rc != 0:
            raise SystemExit(f"rank {rank} step {k} {step['op']} -> {rc}: {L.ncclGetErrorString(rc).decode()}")
    assert L.ncclCommDestroy(comm) == 0
    np.savez(out_path, **out)


if __name__ == "__main__":
    main()
