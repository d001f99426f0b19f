"""Capture-owned arrival counters across a chunk boundary (csrc/runtime.hip: ticket_slot), in a process that has captured nothing
before -- the counters are process-wide, so only here are the counts exact.  Run by
tests/test_gpu_replay.py::test_capture_owned_counters_across_a_chunk_boundary; prints REPLAY_COUNTERS_OK and exits 0, or raises.

fx3d_chamfer_fwd at 64 x 64 x 2, D = 3 takes the small-problem kernel (the plan says kernel=tiny), and that route takes a counter
(csrc/chamfer_host.hip: the ``NN1_F16 || NN1_TINY`` branch).  Call i uses the weights (i + 1, 1) and writes loss[i]; all calls
of one graph share one workspace.  A capturing call takes the next of kCapChunk = 4096 capture-owned slots; an EAGER call that
sees more than half of the chunk used sets up a spare chunk; a capturing call that finds the chunk full moves on to the spare,
and without one it is refused before anything is launched: FX3D_ERR_HIP, "no capture-owned arrival counter left: run the captured
sequence once eagerly before capturing".  Neither the library nor the loader treats that status as a lost context (it is a plain
return; only the drivers of tests/abi_families.py end the session on it, because there it can only mean a fault), so the
process goes on after it.

  1  eager calls for every weight used below: the reference values (the first of them sets the chunk up; none of them changes a
     count, no capture-owned slot being in use yet); a sample of them within LOSS_RTOL of oracle.chamfer_distance
  2  record G1, 2049 calls (slots 0 .. 2048), replay it
  3  one eager call: more than half of the chunk is used, so this one sets up the spare
  4  record G2, 2049 calls: slots 2049 .. 4095, then the first two of the spare
  5  replay G1, G2, G1: every loss bit-equal to its eager value
  6  with no eager call in between, record until the library refuses: the spare holds 4096, two are used, so 4094 more calls are
     recorded and the next -- the 8193rd captured call of the process -- is refused, with the documented status and a message that
     names the remedy
  7  end that capture; its replay gives the 4094 recorded losses and leaves the refused call's loss untouched (nothing was
     recorded for it); destroy it
  8  one eager call: FX3D_OK, the right loss (and the spare the next capture needs)
  9  a new capture of one call succeeds and replays correctly"""
import ctypes as C
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE]

import flux3d_jl_amd as fx  # noqa: E402
from oracle import oracle  # noqa: E402
from test_gpu_hardening import LOSS_RTOL  # noqa: E402

N, M, B, D = 64, 64, 2, 3
CHUNK = 4096        # csrc/runtime.hip: kCapChunk
PER_GRAPH = CHUNK // 2 + 1
ERR_HIP = -2


def main():
    lib = fx._lib
    buf = C.create_string_buffer(512)
    lib.call("fx3d_nn1_plan_describe", N, M, B, D, buf, 512)
    assert "kernel=tiny" in buf.value.decode().split(), buf.value
    rng = np.random.default_rng(5)
    xh, yh = (np.asfortranarray(rng.random((D, n, B), dtype=np.float32)) for n in (N, M))
    x, y = fx.gpu(xh), fx.gpu(yh)
    nb = lib.query_bytes("fx3d_chamfer_workspace_bytes", N, M, B, D)
    st = fx.Stream.create()
    last = 2 * CHUNK - 2 * PER_GRAPH     # the call of step 6 that must be refused: 4094 (0-based)
    ones = np.full(last + 1, 0xFFFFFFFF, np.uint32).view(np.float32)

    def losses():
        return fx.gpu(ones)

    def scratch():
        return fx.DeviceArray.zeros((max(nb, 256),), np.uint8)

    def call(i, loss, ws):
        return lib.load().fx3d_chamfer_fwd(x.ptr, N, y.ptr, M, B, D, float(i + 1), 1.0, loss.ptr + 4 * i, None, None, None, ws.ptr, nb, st.handle)

    def record(count, loss, ws):
        """(graph, the calls recorded, the status of the call that ended the recording)."""
        lib.call("fx3d_graph_begin_capture", st.handle)
        made, rc = 0, 0
        try:
            while made < count:
                rc = call(made, loss, ws)
                if rc:
                    break
                made += 1
        finally:
            h = C.c_void_p()
            lib.call("fx3d_graph_end_capture", st.handle, C.byref(h))
        return h, made, rc

    def replay(g, loss, count, what):
        loss.copy_(ones)
        lib.call("fx3d_graph_launch", g, st.handle)
        st.synchronize()
        got = loss.to_host().view(np.uint32)
        assert np.array_equal(got[:count], eager[:count]), (what, np.flatnonzero(got[:count] != eager[:count])[:5])
        assert np.all(got[count:] == 0xFFFFFFFF), (what, "a loss behind the recorded calls was written")

    def one_eager(i, what):
        loss, ws = losses(), scratch()
        assert call(i, loss, ws) == 0, (what, lib.last_error())
        st.synchronize()
        assert loss.to_host().view(np.uint32)[i] == eager[i], what

    # 1
    le, we = losses(), scratch()
    for i in range(last + 1):
        assert call(i, le, we) == 0, lib.last_error()
    st.synchronize()
    eager = le.to_host().view(np.uint32)
    for i in (0, 1, PER_GRAPH - 1, last):
        want = oracle.chamfer_distance(xh, yh, float(i + 1), 1.0)
        assert np.isclose(eager.view(np.float32)[i], want, rtol=LOSS_RTOL, atol=0), (i, eager.view(np.float32)[i], want)
    # 2
    l1, w1 = losses(), scratch()
    g1, made, rc = record(PER_GRAPH, l1, w1)
    assert (made, rc) == (PER_GRAPH, 0), (made, rc, lib.last_error())
    replay(g1, l1, PER_GRAPH, "G1")
    # 3
    one_eager(7, "the eager call that sets up the spare")
    # 4
    l2, w2 = losses(), scratch()
    g2, made, rc = record(PER_GRAPH, l2, w2)
    assert (made, rc) == (PER_GRAPH, 0), (made, rc, lib.last_error())
    # 5
    replay(g1, l1, PER_GRAPH, "G1 after G2 was recorded")
    replay(g2, l2, PER_GRAPH, "G2, across the chunk boundary")
    replay(g1, l1, PER_GRAPH, "G1 again")
    # 6
    l3, w3 = losses(), scratch()
    g3, made, rc = record(last + 1000, l3, w3)
    msg = lib.last_error()
    assert made == last, (made, last, "the refusal must arrive at the 8193rd captured call of the process")
    assert rc == ERR_HIP and "no capture-owned arrival counter left" in msg and "eagerly before capturing" in msg, (rc, msg)
    # 7
    assert g3.value, "the capture that held the refused call did not end in a graph"
    replay(g3, l3, last, "G3: the calls recorded before the refusal, and nothing for the refused one")
    lib.call("fx3d_graph_destroy", g3)
    # 8
    one_eager(11, "an eager call after the refusal")
    # 9
    l4, w4 = losses(), scratch()
    g4, made, rc = record(1, l4, w4)
    assert (made, rc) == (1, 0), (made, rc, lib.last_error())
    replay(g4, l4, 1, "a capture after the refusal")
    replay(g1, l1, PER_GRAPH, "G1 at the end")
    for g in (g1, g2, g4):
        lib.call("fx3d_graph_destroy", g)
    print(f"eager {last + 1} calls; G1, G2 {PER_GRAPH} each; G3 refused at its call {last + 1}; REPLAY_COUNTERS_OK")


if __name__ == "__main__":
    main()
