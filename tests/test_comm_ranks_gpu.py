"""The frame gather behind the C ABI (csrc/bgs_comm.hip, bgs_comm_*) with MORE THAN ONE RANK, on the one device every box has:
libbgs opens the tests' stand-in for librccl (BGS_RCCL_LIBRARY -> tests/host_shim/fake_rccl.cpp), which performs a real
gather between the communicator streams of one process — real streams, events and device copies, the bytes ordered on the
device as RCCL orders them. One GaussianSplattingPlugin(0) per rank. What this reaches and tests/test_native_gather.py
(one rank, the real RCCL) cannot: a root other than 0, a non-root rank with its NULL receive buffer, the rank-major receive
block, the ticket ring wrapping, a wait on a ticket older than the ring, the error returns of ncclCommInitRank and
ncclGather, and bgs_comm_gather_after ordering a rank's send behind that rank's frames in flight. The gather over a real
link between two devices stays with the skipped two-rank tests of tests/test_native_gather.py.

Every test runs in a freshly spawned child: g_rccl (which librccl the process holds) is process-wide, and the pytest
process may hold the real one. The stand-in never blocks: the ranks of a collective are driven from one thread, the root
last. Its one difference from RCCL — a sender's call is complete at once, not when the root has read the block — is why a
send buffer is only rewritten after the ROOT's ticket was waited for."""
import ctypes
import json
import os
import time

import numpy as np
import pytest

import fake_rccl

pytestmark = pytest.mark.gpu

RING = 16                      # bgs_comm::RING (csrc/bgs_comm.hip): the tickets an event ring remembers
BGS_EINVAL, BGS_EHIP = -1, -3  # include/bgs.h
W, H, FRAMES, BATCH = 320, 180, 11, 4


# ---- the child's side ------------------------------------------------------------------------------------------------

def _child(name, outdir, library, args):
    os.environ["BGS_RCCL_LIBRARY"] = library   # before the first bgs_comm_* call: rccl_api() reads it once
    os.environ["BGS_QUEUE_HOLDERS"] = "0"
    t0 = time.perf_counter()
    result = globals()[name](*args) or {}
    result["seconds"] = time.perf_counter() - t0
    with open(os.path.join(outdir, "result.json"), "w") as f:
        json.dump(result, f)


def _pattern(rank, k, n):
    """f(rank, k, i): the byte rank `rank` sends at offset i of collective k (no period of 256 along i)."""
    i = np.arange(n, dtype=np.uint32)
    return (i * 7 + (i >> 8) * 31 + rank * 59 + k * 101).astype(np.uint8)


def _open_ranks(world):
    """world contexts on device 0, one communicator each over the stand-in: (stand-in, plugins, id, communicators)."""
    from bevy_gaussian_splatting_amd import GaussianSplattingPlugin
    fake = fake_rccl.load()
    plugs = [GaussianSplattingPlugin(0) for _ in range(world)]
    uid = plugs[0].comm_unique_id()
    assert len(uid) == 128 and uid[:8] == b"FAKERCCL", "libbgs did not open the stand-in"
    live0 = fake.fake_rccl_live_comms()
    comms = [plugs[r].comm_create(uid, world, r) for r in range(world)]
    assert all(comms) and fake.fake_rccl_live_comms() == live0 + world
    return fake, plugs, uid, comms


def _close_ranks(fake, plugs, comms):
    for p, c in zip(plugs, comms):
        p.comm_destroy(c)
    for p in plugs:
        p.close()
    assert fake.fake_rccl_live_comms() == 0 and fake.fake_rccl_pending_posts() == 0


def _gather_all(plugs, comms, root, send, n, recv):
    """One collective: the senders, then the root. Returns the tickets by rank."""
    world = len(plugs)
    tickets = [0] * world
    for r in [r for r in range(world) if r != root] + [root]:
        tickets[r] = plugs[r].comm_gather(comms[r], root, send[r], n, recv if r == root else None)   # a sender's recv is NULL
    return tickets


def _upload_patterns(plugs, send, k, n):
    for r, p in enumerate(plugs):
        p.upload_bytes(send[r], _pattern(r, k, n))


def _expect_block(plug, recv, world, k, n, guard, what):
    back = np.empty(world * n + guard, np.uint8)
    plug.download(recv, back)
    for r in range(world):
        assert np.array_equal(back[r * n:(r + 1) * n], _pattern(r, k, n)), f"{what}: rank {r}'s block of collective {k} is not at {r} * {n}"
    assert (back[world * n:] == 0xC3).all(), f"{what}: the bytes behind the receive block were written"


def raw_seam():
    world, n, guard, total = 4, 4097, 256, 40
    fake, plugs, uid, comms = _open_ranks(world)
    send = [p.device_alloc(n) for p in plugs]
    recv = {root: plugs[root].device_alloc(world * n + guard) for root in (0, 3)}
    for root, ptr in recv.items():
        plugs[root].upload_bytes(ptr, np.full(world * n + guard, 0xC3, np.uint8))
    streams = []
    for p, c in zip(plugs, comms):
        s = ctypes.c_void_p()
        assert p._lib.bgs_comm_stream(p._ctx, c, ctypes.byref(s)) == 0 and s.value
        streams.append(s.value)
    assert len(set(streams)) == world
    for k in range(total):
        root = 0 if k % 2 == 0 else 3
        _upload_patterns(plugs, send, k, n)
        tickets = _gather_all(plugs, comms, root, send, n, recv[root])
        assert tickets == [k + 1] * world, (k, tickets)
        info = fake_rccl.comm_info(fake, uid, root)
        assert (info.last_datatype, info.last_root, info.last_count, info.last_stream, info.last_result) == \
               (fake_rccl.NCCL_UINT8, root, n, streams[root], 0), k
        assert info.gather_calls == info.gathers_completed == k + 1
        if k < total - 1:   # (the root's ticket: the senders' buffers are free again, this gather's bytes are in place)
            plugs[root].comm_wait(comms[root], tickets[root])
            _expect_block(plugs[root], recv[root], world, k, n, guard, f"gather {k}")
    # after the 40th gather, on its root: a ticket RING - 1 back is still in the ring, one RING back is not (the stream is
    # synchronised instead: that wait alone puts the 40th gather's bytes in place), then the newest ticket and ticket 0
    k, root = total - 1, 3
    plugs[root].comm_wait(comms[root], total - (RING - 1))
    plugs[root].comm_wait(comms[root], total - RING)
    _expect_block(plugs[root], recv[root], world, k, n, guard, "ticket RING back")
    for ticket in (total, 0):
        plugs[root].comm_wait(comms[root], ticket)
        _expect_block(plugs[root], recv[root], world, k, n, guard, f"ticket {ticket}")
    for r in range(world):   # a sender's tickets wait too, and none was handed out beyond the 40th
        plugs[r].comm_wait(comms[r], total)
        rc = plugs[r]._lib.bgs_comm_wait(plugs[r]._ctx, comms[r], total + 1)
        assert rc == BGS_EINVAL, rc
    for r, p in enumerate(plugs):
        p.device_free(send[r])
    for root, ptr in recv.items():
        plugs[root].device_free(ptr)
    _close_ranks(fake, plugs, comms)
    return {"gathers": total}


def nothing_to_move():
    world, n, guard = 4, 4097, 256
    fake, plugs, uid, comms = _open_ranks(world)
    send = [p.device_alloc(n) for p in plugs]
    recv = plugs[0].device_alloc(world * n + guard)
    plugs[0].upload_bytes(recv, np.full(world * n + guard, 0xC3, np.uint8))

    def calls():
        return [int(fake_rccl.comm_info(fake, uid, r).gather_calls) for r in range(world)]

    assert _gather_all(plugs, comms, 0, send, 0, recv) == [0] * world and calls() == [0] * world   # before any gather
    _upload_patterns(plugs, send, 0, n)
    assert _gather_all(plugs, comms, 0, send, n, recv) == [1] * world
    plugs[0].comm_wait(comms[0], 1)
    _expect_block(plugs[0], recv, world, 0, n, guard, "gather 0")
    assert _gather_all(plugs, comms, 0, send, 0, recv) == [0] * world and calls() == [1] * world
    for r in reversed(range(world)):   # ... and through bgs_comm_gather_after
        assert plugs[r].comm_gather_after(comms[r], 0, send[r], 0, recv if r == 0 else None) == 0
    assert calls() == [1] * world
    plugs[0].comm_wait(comms[0], 0)
    _expect_block(plugs[0], recv, world, 0, n, guard, "after the empty gathers")   # nothing moved
    _upload_patterns(plugs, send, 1, n)
    assert _gather_all(plugs, comms, 0, send, n, recv) == [2] * world and calls() == [2] * world
    plugs[0].comm_wait(comms[0], 2)
    _expect_block(plugs[0], recv, world, 1, n, guard, "gather 1")
    for r, p in enumerate(plugs):
        p.device_free(send[r])
    plugs[0].device_free(recv)
    _close_ranks(fake, plugs, comms)


def library_errors():
    from bevy_gaussian_splatting_amd import GaussianSplattingPlugin
    from bevy_gaussian_splatting_amd._native import BgsError
    world, n, guard = 4, 4097, 256
    fake, plugs, uid, comms = _open_ranks(world)
    # -- a rank that is taken: ncclCommInitRank's error comes back as BGS_EHIP, no communicator on either side
    with GaussianSplattingPlugin(0) as extra:
        out = ctypes.c_void_p(0xDEAD)
        rc = extra._lib.bgs_comm_create(extra._ctx, uid, world, 2, ctypes.byref(out))
        msg = extra._lib.bgs_last_error(extra._ctx).decode()
        assert rc == BGS_EHIP and "ncclCommInitRank" in msg and "fake rccl: invalid usage" in msg, (rc, msg)
        assert out.value is None and fake.fake_rccl_live_comms() == world
        with pytest.raises(BgsError, match="ncclCommInitRank: fake rccl") as ei:
            extra.comm_create(uid, world + 1, 1)             # a world size the group does not have
        assert ei.value.status == BGS_EHIP and fake.fake_rccl_live_comms() == world
    # -- the root before its senders
    send = [p.device_alloc(n) for p in plugs]
    recv = plugs[0].device_alloc(world * n + guard)
    plugs[0].upload_bytes(recv, np.full(world * n + guard, 0xC3, np.uint8))
    _upload_patterns(plugs, send, 0, n)
    assert _gather_all(plugs, comms, 0, send, n, recv) == [1] * world
    plugs[0].comm_wait(comms[0], 1)
    _upload_patterns(plugs, send, 1, n)

    def root_gather():
        ticket = ctypes.c_uint64(99)
        rc = plugs[0]._lib.bgs_comm_gather(plugs[0]._ctx, comms[0], 0, ctypes.c_void_p(send[0]), n, ctypes.c_void_p(recv), ctypes.byref(ticket))
        return rc, int(ticket.value), plugs[0]._lib.bgs_last_error(plugs[0]._ctx).decode()

    for attempt in range(2):   # (twice: a failure leaves nothing behind that the next call trips over)
        rc, ticket, msg = root_gather()
        assert rc == BGS_EHIP and ticket == 0 and "fake rccl: invalid usage" in msg, (attempt, rc, ticket, msg)
    info = fake_rccl.comm_info(fake, uid, 0)
    assert (info.gather_calls, info.gathers_completed, info.last_result) == (3, 1, fake_rccl.NCCL_INVALID_USAGE)
    plugs[0].comm_wait(comms[0], 1)                                      # the last ticket handed out is still 1 ...
    assert plugs[0]._lib.bgs_comm_wait(plugs[0]._ctx, comms[0], 2) == BGS_EINVAL   # ... and 2 does not exist yet
    _expect_block(plugs[0], recv, world, 0, n, guard, "after the refused gathers")   # "it changes nothing"
    assert plugs[1].comm_gather(comms[1], 0, send[1], n, None) == 2
    rc, ticket, msg = root_gather()                                      # two of three senders: still refused
    assert rc == BGS_EHIP and ticket == 0, (rc, ticket, msg)
    with pytest.raises(BgsError, match="fake rccl: invalid argument") as ei:   # a sender that disagrees on the count
        plugs[2].comm_gather(comms[2], 0, send[2], n - 1, None)
    assert ei.value.status == BGS_EHIP
    assert plugs[2].comm_gather(comms[2], 0, send[2], n, None) == 2      # the refused call took no ticket
    assert plugs[3].comm_gather(comms[3], 0, send[3], n, None) == 2
    rc, ticket, msg = root_gather()
    assert rc == 0 and ticket == 2, (rc, ticket, msg)
    plugs[0].comm_wait(comms[0], 2)
    _expect_block(plugs[0], recv, world, 1, n, guard, "gather 1")
    # ... and the ring's slots still go round in turn: RING + 2 more gathers, each waited for by its own ticket
    for k in range(2, RING + 4):
        _upload_patterns(plugs, send, k, n)
        assert _gather_all(plugs, comms, 0, send, n, recv) == [k + 1] * world
        plugs[0].comm_wait(comms[0], k + 1)
        _expect_block(plugs[0], recv, world, k, n, guard, f"gather {k}")
    # -- teardown
    for r, p in enumerate(plugs):
        p.device_free(send[r])
    plugs[0].device_free(recv)
    _close_ranks(fake, plugs, comms)


def frame_gather(world, dst, device_wait):
    from bevy_gaussian_splatting_amd import CloudSettings, GaussianSplattingPlugin, random_gaussians_3d_seeded
    from bevy_gaussian_splatting_amd.multiview import NativeFrameGather, headless_view
    fake = fake_rccl.load()
    cloud = random_gaussians_3d_seeded(20_000, 2)
    plugs = [GaussianSplattingPlugin(0) for _ in range(world)]
    uid = plugs[0].comm_unique_id()
    assert uid[:8] == b"FAKERCCL", "libbgs did not open the stand-in"
    settings = CloudSettings()
    views = [headless_view(r, W, H) for r in range(world)]
    handles, own = [], []
    for p, v in zip(plugs, views):   # every rank's own frame, blocking, rendered first: the reference bytes
        handles.append(p.upload(cloud))
        p.set_output_srgb8(True)
        p.render(handles[-1], v, settings)
        ptr, nbytes = p.framebuffer_srgb8_device_ptr()
        assert nbytes == W * H * 4
        own.append(p.download(ptr, np.empty((H, W, 4), np.uint8)))
    got = []

    def on_batch(recv_ptr, count):
        blk = np.empty((world, BATCH, H, W, 4), np.uint8)
        plugs[dst].download(recv_ptr, blk)
        got.append(blk[:, :count].copy())

    bgs = [NativeFrameGather(plugs[r], W * H * 4, world, r, uid, batch=BATCH, dst=dst, on_batch=on_batch if r == dst else None,
                             device_wait=device_wait) for r in range(world)]
    assert fake.fake_rccl_live_comms() == world

    def reruns(p):
        c = p.adaptive_counters()
        return c["reruns_sort"] + c["reruns_lists"]

    reruns0 = [reruns(p) for p in plugs]
    for p in plugs:
        p.set_async(True)
        p.set_pipeline_depth(4)
        p.set_packed_only(True)
    root_first = [dst] + [r for r in range(world) if r != dst]
    root_last = root_first[1:] + [dst]
    for _ in range(FRAMES):
        # a staging buffer is handed out again once ITS rank's gather out of it is complete; the stand-in's senders are
        # complete at once, so the root — whose ticket says the block was read — takes its slot first ...
        target = {r: bgs[r].next_target() for r in root_first}
        for r in root_last:   # ... and wherever a batch can leave, the root calls last
            p = plugs[r]
            p.set_srgb8_target(target[r])
            p.render(handles[r], views[r], settings, download=False)
            bgs[r].frame_enqueued()
            if p.frames_in_flight() >= 4:
                p.pipeline_pop()
                bgs[r].frame_completed()
    while plugs[dst].frames_in_flight():
        for r in root_last:
            plugs[r].pipeline_pop()
            bgs[r].frame_completed()
    assert not any(p.frames_in_flight() for p in plugs)
    if device_wait:   # a frame re-run after its batch went out would have been sent stale: none on a settled view
        for r in range(world):
            bgs[r].note_rerun(reruns(plugs[r]) - reruns0[r])
            assert bgs[r].stale_frames == 0
    for r in root_last:
        bgs[r].flush()
    assert bgs[dst].frames_received == world * FRAMES and [g.gathers for g in bgs] == [-(-FRAMES // BATCH)] * world
    assert all(g.frames_received == 0 for r, g in enumerate(bgs) if r != dst)
    for r in range(world):   # the stand-in saw one call per gather and rank, each a whole staging batch to `dst`
        info = fake_rccl.comm_info(fake, uid, r)
        assert (info.gather_calls, info.gathers_completed, info.last_root, info.last_count, info.last_datatype) == \
               (3, 3, dst, BATCH * W * H * 4, fake_rccl.NCCL_UINT8)
    allf = np.concatenate(got, axis=1)
    assert allf.shape == (world, FRAMES, H, W, 4)
    for r in range(world):
        assert own[r].any()
        for k in range(FRAMES):
            assert np.array_equal(allf[r, k], own[r]), f"rank {r}, frame {k}: not the frame the rank rendered on its own"
    for a in range(world):
        for b in range(a + 1, world):
            assert not np.array_equal(own[a], own[b]), f"cameras {a} and {b} rendered the same frame"
    for p in plugs:
        p.set_async(False)
        p.set_packed_only(False)
    for g in bgs:
        g.close()
    for h in handles:
        h.free()
    for p in plugs:
        p.close()
    assert fake.fake_rccl_live_comms() == 0 and fake.fake_rccl_pending_posts() == 0
    return {"frames_received": bgs[dst].frames_received, "gathers": bgs[dst].gathers}


def device_side_wait():
    from bevy_gaussian_splatting_amd import CloudSettings, GaussianSplattingPlugin, random_gaussians_3d_seeded
    from bevy_gaussian_splatting_amd.multiview import NativeFrameGather, headless_view
    fake = fake_rccl.load()
    w, h = 1920, 1080
    nbytes = w * h * 4
    root, sender = GaussianSplattingPlugin(0), GaussianSplattingPlugin(0)
    uid = root.comm_unique_id()
    assert uid[:8] == b"FAKERCCL", "libbgs did not open the stand-in"
    cloud, view, settings = random_gaussians_3d_seeded(200_000, 2), headless_view(1, w, h), CloudSettings()
    handle = sender.upload(cloud)
    sender.set_output_srgb8(True)
    sender.render(handle, view, settings)                      # blocking: the bytes the root must end up with
    ptr, size = sender.framebuffer_srgb8_device_ptr()
    assert size == nbytes
    own = sender.download(ptr, np.empty((h, w, 4), np.uint8))
    assert own.any() and (own != 0xA5).any()
    got = []

    def on_batch(recv_ptr, count):
        got.append(root.download(recv_ptr, np.empty((2, 1, h, w, 4), np.uint8)))
        assert count == 1

    bg0 = NativeFrameGather(root, nbytes, 2, 0, uid, batch=1, dst=0, on_batch=on_batch, device_wait=True)
    bg1 = NativeFrameGather(sender, nbytes, 2, 1, uid, batch=1, dst=0, device_wait=True)
    sender.set_async(True)
    sender.set_pipeline_depth(4)
    sender.set_packed_only(True)
    for _ in range(4):   # every lane has run a frame of this view: the frame below allocates nothing, learns nothing
        sender.render(handle, view, settings, download=False)
    while sender.frames_in_flight():
        sender.pipeline_pop()
    c = sender.adaptive_counters()
    reruns0 = c["reruns_sort"] + c["reruns_lists"]
    t0, t1 = bg0.next_target(), bg1.next_target()
    root.upload_bytes(t0, np.full(nbytes, 0x3C, np.uint8))
    sender.upload_bytes(t1, np.full(nbytes, 0xA5, np.uint8))   # what a gather that did not wait would deliver
    sender.set_srgb8_target(t1)
    sender.render(handle, view, settings, download=False)      # enqueued ...
    bg1.frame_enqueued()                                       # ... and handed to the communicator at once: no pop, no wait
    assert sender.frames_in_flight() == 1 and bg1.gathers == 1
    bg0.frame_enqueued()                                       # the root: its copies go behind the sender's event
    bg0.flush()                                                # the root's ticket; the sender's frame was never waited for
    assert sender.frames_in_flight() == 1 and len(got) == 1
    sender.pipeline_pop()
    c = sender.adaptive_counters()
    assert c["reruns_sort"] + c["reruns_lists"] == reruns0, "the frame was re-run after its batch had left: not this test's case"
    assert (got[0][0, 0] == 0x3C).all(), "the root's own block"
    filled = float((got[0][1, 0] == 0xA5).all(axis=-1).mean())
    assert np.array_equal(got[0][1, 0], own), f"the root did not get the rendered frame ({filled:.0%} of its pixels are the fill)"
    bg1.flush()
    sender.set_async(False)
    sender.set_packed_only(False)
    bg1.close()
    bg0.close()
    handle.free()
    sender.close()
    root.close()
    assert fake.fake_rccl_live_comms() == 0 and fake.fake_rccl_pending_posts() == 0


def no_library(library, expect):
    from bevy_gaussian_splatting_amd import GaussianSplattingPlugin
    from bevy_gaussian_splatting_amd._native import BgsError
    assert os.environ["BGS_RCCL_LIBRARY"] == library
    messages = []
    for _ in range(2):   # the second call tries again, and fails the same way
        with pytest.raises(BgsError) as ei:
            GaussianSplattingPlugin.comm_unique_id()
        assert ei.value.status == BGS_EHIP
        messages.append(str(ei.value))
    with GaussianSplattingPlugin(0) as p:   # ... and with a context: the message is the context's
        with pytest.raises(BgsError) as ei:
            p.comm_create(bytes(128), 1, 0)
        assert ei.value.status == BGS_EHIP
        messages.append(str(ei.value))
    for m in messages:
        assert all(e in m for e in expect), (m, expect)
    return {"message": messages[0]}


# ---- the tests -------------------------------------------------------------------------------------------------------

def _run_child(tmp_path, name, *args, library=None, timeout=120):
    import multiprocessing as mp
    library = fake_rccl.build() if library is None else library
    proc = mp.get_context("spawn").Process(target=_child, args=(name, str(tmp_path), library, args))
    proc.start()
    proc.join(timeout)
    if proc.is_alive():
        proc.kill()
        proc.join()
        pytest.fail(f"{name}: the child did not finish in {timeout} s")
    assert proc.exitcode == 0, f"{name}: the child exited with {proc.exitcode} (its output is above)"
    with open(tmp_path / "result.json") as f:   # written by the child's last statement: it ran to its end
        return json.load(f)


def test_raw_seam_world_4_alternating_roots_and_ring_wrap(tmp_path):
    """40 gathers of 4097 bytes per rank between four ranks, the root 0 and 3 in turn: the root's block is the four ranks'
    patterns in rank order, byte for byte, with the guard behind it intact; tickets run 1..40 on every rank (a sender's
    receive pointer is NULL); the stand-in saw ncclUint8, the root, the count and bgs_comm_stream's stream. 40 > 2 * RING:
    every event slot is recorded again, half of them twice. After the last gather bgs_comm_wait returns for the newest ticket, one
    RING - 1 back, one RING back (the stream-synchronise branch) and ticket 0; ticket 41 is BGS_EINVAL."""
    assert _run_child(tmp_path, "raw_seam")["gathers"] == 40


def test_nothing_to_move_takes_no_ticket_and_no_collective(tmp_path):
    """bytes_per_rank == 0 on all four ranks: ticket 0 and not one ncclGather call, through bgs_comm_gather and
    bgs_comm_gather_after, before any gather and between two; the next gather has the next ticket and the right bytes."""
    _run_child(tmp_path, "nothing_to_move")


def test_errors_of_the_library_come_back_and_leave_no_trace(tmp_path):
    """ncclCommInitRank refusing a rank that is taken: BGS_EHIP with the call's name and the library's text, *out NULL,
    no communicator left in the library. ncclGather refusing the root that calls before its senders: BGS_EHIP, ticket 0;
    once the senders have posted the same call takes the ticket after the last successful one, its bytes are right, and
    RING + 2 further gathers each complete under their own ticket (a failure neither advanced the count nor used an
    event slot out of turn). After the four communicators and contexts are gone the library holds no communicator."""
    _run_child(tmp_path, "library_errors")


@pytest.mark.parametrize("device_wait", [False, True])
@pytest.mark.parametrize("dst", [0, 3])
def test_native_frame_gather_world_4(tmp_path, dst, device_wait):
    """NativeFrameGather end to end between four ranks on one device: 20 k splats at 320x180, camera r on rank r, 11 frames
    in batches of 4 (two full, one partial), packed-only sRGB8, four frames in flight. For every rank and frame the root
    holds exactly that rank's own blocking frame; the four cameras' frames differ pairwise; 44 frames in 3 gathers; no
    stale frame with the device-side wait."""
    got = _run_child(tmp_path, "frame_gather", 4, dst, device_wait)
    assert got["frames_received"] == 44 and got["gathers"] == 3


def test_native_frame_gather_world_8(tmp_path):
    """The same with BASELINE configs[4]'s rank count: eight contexts, eight cameras, root 0, the device-side wait."""
    got = _run_child(tmp_path, "frame_gather", 8, 0, True)
    assert got["frames_received"] == 88 and got["gathers"] == 3


def test_gather_after_sends_the_frame_not_what_was_there_before(tmp_path):
    """bgs_comm_gather_after orders a rank's send behind that rank's frames in flight: rank 1 enqueues one 1920x1080 frame
    of 200 k splats into a target filled with 0xA5 and hands the gather over at once, with no host wait in between; the
    root's copy of rank 1's block waits on the device (the event the stand-in records on rank 1's communicator stream
    stands behind the lane's) and holds the rendered frame, not the fill.

    This shows the ordering only as far as a race can: without the wait the copy would start while the frame — a few
    hundred microseconds of device time — has barely begun, so the fill would be LIKELY, not certain, to arrive. The test
    cannot fail for a correct library; it can pass for a broken one."""
    _run_child(tmp_path, "device_side_wait")


def test_a_library_that_does_not_exist_is_reported_by_name(tmp_path):
    """BGS_RCCL_LIBRARY is the only name tried: a file that does not exist is BGS_EHIP, `librccl not found: ` with the
    loader's text, which names the file — on every call (rccl_api stays retryable), and the process lives. (The message
    used to be built from a second dlerror(), which returns NULL: std::string + nullptr, a crash.)"""
    missing = str(tmp_path / "libno_such_rccl.so")
    got = _run_child(tmp_path, "no_library", missing, ["librccl not found", missing], library=missing)
    assert "libno_such_rccl.so" in got["message"]


def test_a_library_without_the_symbols_is_refused(tmp_path):
    """Another of the project's shims behind BGS_RCCL_LIBRARY: it opens, has none of the five symbols, and is refused."""
    import helpers
    helpers.shim()
    got = _run_child(tmp_path, "no_library", helpers.SHIM_LIB, ["librccl lacks ncclGetUniqueId"], library=helpers.SHIM_LIB)
    assert "librccl lacks" in got["message"]
