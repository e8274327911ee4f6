"""The engine session (csrc/tz_tei.cpp, api.Tei) and examples/tei_cli.cpp against a restatement of tei/src/main.rs:139-297 written
here over api.BatchedMCTS on a second net of the same tensors (class Restated): set_positions / play_moves, one simulate at
creation, step() for tree reuse, simulate_batch(rounds=1) until the visit condition, principal_variation, select_best_actions.
Of an info line `nodes`, the score fields and `pv` are compared (time and nps are the clock's); the info interval is set very large
so that a search sends exactly one info line."""
import os
import re
import subprocess
import threading
import time

import numpy as np
import pytest

from gpu_util import require_gpu

pytestmark = pytest.mark.gpu

HUGE_INTERVAL = 10 ** 9
INFO = re.compile(r"^info time (\d+) nodes (\d+) nps (\d+) (wdl .*)$")
SEED = {4: 41, 5: 52}


def _weights(n):
    from takzero_amd import weights as W

    return W.init_weights(W.ARCH_TEST, n=n, blocks=2, seed=SEED[n])


def _net(A, n):
    return A.Net(arch=A.ARCH_TEST, n=n, precision=A.PREC_F16, blocks=2).load_tensors(_weights(n))


def _start_tps(n):
    return "/".join(["x%d" % n] * n) + " 1 1"


class Restated:
    """tei/src/main.rs:139-297 over BatchedMCTS, with the session's documented departures (teinewgame forgets the last position)"""

    def __init__(self, A, n, leaves, capacity=0):
        self.A, self.n, self.leaves = A, n, leaves
        self.m = A.BatchedMCTS(1, n, 4, agent=_net(A, n), node_capacity=capacity)
        self.zero = np.zeros(1, np.float32)
        self.m.set_positions([0], [A.state_from_tps(_start_tps(n), n, 4)])
        self.m.simulate(self.zero, 1)                                  # node.simulate_simple, main.rs:141
        self.last = ("startpos", [])

    def newgame(self):
        self.m.set_positions([0], [self.A.state_from_tps(_start_tps(self.n), self.n, 4)])
        self.last = None

    def position(self, tps, moves):
        """tps None = startpos; moves in PTN"""
        key = tps or "startpos"
        if self.last is not None and self.last[0] == key and moves[:len(self.last[1])] == self.last[1]:
            for mv in moves[len(self.last[1]):]:                       # tree reuse, main.rs:175-184
                a = np.array([self.A.move_from_ptn(self.n, mv)], np.uint16)
                if self.m.root_info()["n_children"][0] > 0:
                    self.m.step(a)
                else:
                    assert self.m.play_moves(a)[0] == 1
        else:
            self.m.set_positions([0], [self.A.state_from_tps(tps or _start_tps(self.n), self.n, 4)])
            for mv in moves:
                assert self.m.play_moves(np.array([self.A.move_from_ptn(self.n, mv)], np.uint16))[0] == 1
        self.last = (key, list(moves))

    def go_nodes(self, nodes):
        """main.rs:251-290 -> (nodes of the info line, its fields from wdl on, bestmove)"""
        at_start = int(self.m.root_info()["visit_count"][0])
        while True:
            self.m.simulate_batch(self.zero, self.leaves, 1)
            visits = int(self.m.root_info()["visit_count"][0]) - at_start
            if visits >= nodes:
                break
        info = self.m.root_info()[0]
        line = self.A.tei_format_info(self.n, 1, visits, info["eval_tag"], info["eval_bits"], self.m.principal_variation(0))
        return visits, INFO.match(line).group(4), self.A.move_to_ptn(self.n, int(self.m.select_best_actions()[0]))


def _engine(A, n, leaves, capacity=0, sink=None):
    mcts = A.BatchedMCTS(1, n, 4, agent=_net(A, n), node_capacity=capacity)
    tei = A.Tei(mcts, leaves=leaves, sink=sink)
    tei.set_info_interval(HUGE_INTERVAL)
    return mcts, tei


def _go(tei, command):
    """(nodes, fields from wdl on, bestmove, time in ms) of a search that sent exactly one info line"""
    lines = tei.line(command)
    infos = [INFO.match(l) for l in lines if l.startswith("info time")]
    best = [l.split()[1] for l in lines if l.startswith("bestmove ")]
    assert len(infos) == 1 and infos[0] and len(best) == 1 and lines[-1].startswith("bestmove "), lines
    assert int(infos[0].group(3)) == (1000 * int(infos[0].group(2)) // int(infos[0].group(1)) if int(infos[0].group(1)) else 0)
    return int(infos[0].group(2)), infos[0].group(4), best[0], int(infos[0].group(1))


TPS = {4: "x4/x,1,2,x/x,2,1,x/x4 1 3", 5: "x5/x,1,2,x2/x2,1,x2/x,2,x2,1/x5 2 3"}


@pytest.mark.parametrize("n, leaves", [(4, 8), (5, 16)])
def test_go_nodes_equals_the_restatement(n, leaves):
    """N below, equal to and above a multiple of the leaves a round adds; after `position startpos` on the session's first tree (one
    simulation), after `position startpos moves ...` (tree reuse from that tree, then from a new game) and after `position tps ...`"""
    A = require_gpu()
    mcts, tei = _engine(A, n, leaves)
    ref = Restated(A, n, leaves)
    assert tei.line("isready") == ["readyok"]
    script = [(None, [], 3 * leaves - 1), ("new", None, 0), (None, ["a1"], 3 * leaves), ("new", None, 0), (None, ["a1", "b2", "c3"], 3 * leaves + 1),
              ("new", None, 0), (TPS[n], [], 2 * leaves - 1), (TPS[n], ["a1"], 2 * leaves), ("new", None, 0), (TPS[n], ["a1", "d4"], 2 * leaves + 1)]
    first = True
    for tps, moves, nodes in script:
        if tps == "new":
            assert tei.line("teinewgame %d" % n) == []
            ref.newgame()
            continue
        if first:                               # the tree of tz_tei_create: the start position after one simulation
            assert mcts.root_info()["visit_count"][0] == 1 == ref.m.root_info()["visit_count"][0]
            first = False
        command = "position " + ("tps " + tps if tps else "startpos") + (" moves " + " ".join(moves) if moves else "")
        assert tei.line(command) == [], command
        ref.position(tps, moves)
        assert mcts.get_positions().tobytes() == ref.m.get_positions().tobytes(), command
        assert mcts.root_info()["visit_count"][0] == ref.m.root_info()["visit_count"][0], command
        got = _go(tei, "go nodes %d" % nodes)
        want = ref.go_nodes(nodes)
        assert got[:3] == want, (command, nodes, got, want)
        assert got[0] >= nodes
    assert mcts.pool_overflows() == 0


def test_tree_reuse_fresh_trees_and_new_games():
    A = require_gpu()
    n, leaves, nodes = 5, 16, 40 * 16
    mcts, tei = _engine(A, n, leaves)
    ref = Restated(A, n, leaves)
    assert tei.line("position startpos moves a1") == []
    ref.position(None, ["a1"])
    got, want = _go(tei, "go nodes %d" % nodes), ref.go_nodes(nodes)
    assert got[:3] == want
    pv = got[1].split(" pv ")[1].split()
    assert len(pv) >= 2, got
    moves = ["a1", pv[0], pv[1]]
    assert pv[0] == got[2]
    # the kept subtree: the engine (tz_search_step_wide) and the restatement (step) hold the same root
    assert tei.line("position startpos moves " + " ".join(moves)) == []
    ref.position(None, moves)
    kept = int(ref.m.root_info()["visit_count"][0])
    assert kept > 0 and mcts.root_info().tobytes() == ref.m.root_info().tobytes()
    got, want = _go(tei, "go nodes %d" % nodes), ref.go_nodes(nodes)
    assert got[:3] == want
    # a move list that does not extend the last one: a fresh tree
    other = ["a1", "e5"] if pv[0] != "e5" else ["a1", "d5"]
    assert tei.line("position startpos moves " + " ".join(other)) == []
    ref.position(None, other)
    assert mcts.root_info()["visit_count"][0] == 0 == ref.m.root_info()["visit_count"][0]
    got, want = _go(tei, "go nodes %d" % (2 * leaves)), ref.go_nodes(2 * leaves)
    assert got[:3] == want
    # after teinewgame the same list as before starts from a fresh tree as well (the reference would extend the old list)
    assert tei.line("position startpos moves " + " ".join(moves)) == []
    assert tei.line("teinewgame %d" % n) == []
    assert tei.line("position startpos moves " + " ".join(moves + ["e1"])) == []
    ref.newgame()
    ref.position(None, moves + ["e1"])
    assert mcts.root_info()["visit_count"][0] == 0
    assert mcts.get_positions().tobytes() == ref.m.get_positions().tobytes()
    got, want = _go(tei, "go nodes %d" % (2 * leaves)), ref.go_nodes(2 * leaves)
    assert got[:3] == want


def test_a_move_onto_a_childless_root_and_illegal_moves():
    A = require_gpu()
    n, leaves = 4, 8
    mcts, tei = _engine(A, n, leaves)
    assert tei.line("teinewgame 4") == [] and tei.line("position startpos") == []
    assert mcts.root_info()["n_children"][0] == 0
    # the root has no children: the move is validated and played, the tree stays empty (Node::descend on a childless node)
    assert tei.line("position startpos moves a1") == []
    assert A.state_to_tps(mcts.get_positions()[0]) == "x4/x4/x4/2,x3 2 1" and mcts.root_info()["visit_count"][0] == 0
    # ... and an illegal one is refused there: a1 is taken
    assert tei.line("position startpos moves a1 a1") == ["info string error: could not play move a1"]
    assert A.state_to_tps(mcts.get_positions()[0]) == "x4/x4/x4/2,x3 2 1"
    # the session goes on: the next position is replayed from the start
    assert tei.line("position startpos moves a1 b1") == []
    assert A.state_to_tps(mcts.get_positions()[0]) == "x4/x4/x4/2,1,x2 1 2"
    nodes, _, best, _ = _go(tei, "go nodes 24")
    assert nodes >= 24 and mcts.root_info()["n_children"][0] > 0
    # on a root with children a move outside them is refused the same way, and the tree and position stay
    before = mcts.root_info().tobytes()
    assert tei.line("position startpos moves a1 b1 b1") == ["info string error: could not play move b1"]
    assert mcts.root_info().tobytes() == before and A.state_to_tps(mcts.get_positions()[0]) == "x4/x4/x4/2,1,x2 1 2"
    assert tei.line("position startpos moves a1 b1 " + best) == []
    assert mcts.root_info()["visit_count"][0] == 0                      # replayed from the start: the failed replay forgot the list
    assert _go(tei, "go nodes 8")[0] >= 8
    # unparsable input leaves the session as it is
    with pytest.raises(A.TakzeroError):
        tei.line("go nodes")
    assert tei.last_lines == ["info string error: parse error: missing the amount of nodes after `go nodes`"]
    assert tei.line("setoption name model value x.ot") == ["info string warning: it's too late to specify options"]
    assert tei.line("stop") == [] and not tei.quit
    assert tei.line("quit") == [] and tei.quit


def test_go_on_a_finished_game_gives_no_bestmove():
    A = require_gpu()
    mcts, tei = _engine(A, 4, 8)
    with pytest.raises(A.TakzeroError) as e:
        tei.line("position tps 1,1,1,1/2,2,2,x/x4/x4 2 4")
        tei.line("go nodes 10")
    assert e.value.code == -6 and tei.last_lines == ["info string error: the position has no moves to search"]    # TZ_ESTATE
    assert tei.line("position startpos") == [] and _go(tei, "go nodes 8")[0] >= 8


def test_the_clock_of_the_side_to_move_sets_the_move_time():
    A = require_gpu()
    n, leaves = 4, 8
    mcts, tei = _engine(A, n, leaves, capacity=1 << 22)
    t0 = time.monotonic()
    nodes, _, best, ms = _go(tei, "go wtime 1000 winc 200 btime 1 binc 1 nodes 1000000000")    # white to move: 1000 / 10 + 3 * 200 / 4 = 250 ms
    elapsed = time.monotonic() - t0
    assert ms >= 250 and elapsed >= 0.25 and nodes < 1000000000 and best
    # the limits are cleared after a search, and the other side's clock alone is no limit: `nodes` ends this one at once
    ref = Restated(A, n, leaves, capacity=1 << 22)
    assert tei.line("teinewgame 4") == [] and tei.line("position startpos") == []
    ref.newgame()
    ref.position(None, [])
    lines = tei.line("go btime 100000 binc 100000 nodes 20")
    assert lines[0] == "info string warning: ignored `go` options of the side not to move"
    got = INFO.match(lines[1])
    assert int(got.group(2)) == ref.go_nodes(20)[0] and lines[2].startswith("bestmove ")


def test_go_infinite_ends_when_the_node_pool_is_nearly_full():
    """3x3, dummy agent, a few thousand slots: the search ends by itself before a round could overflow the pool.  So does one whose
    only limits are the other side's clock."""
    A = require_gpu()
    mcts = A.BatchedMCTS(1, 3, 0, node_capacity=3000)
    tei = A.Tei(mcts, leaves=8)
    tei.set_info_interval(HUGE_INTERVAL)
    timed_out = []
    for command in ("go infinite", "go btime 10 binc 0"):
        assert tei.line("teinewgame 3") == [] and tei.line("position startpos") == []
        guard = threading.Timer(60, lambda: (timed_out.append(command), tei.stop()))
        guard.start()
        lines = tei.line(command)
        guard.cancel()
        assert not timed_out, timed_out
        assert "info string node pool full" in lines and lines[-1].startswith("bestmove ") and lines[-2].startswith("info time "), lines
        used, cap = mcts.pool_usage()
        assert cap == 3000 and cap - used < 8 * 64 and mcts.pool_overflows() == 0
    assert "info string warning: no understood stopping condition given" in lines


def test_stop_from_a_second_thread_ends_go_infinite():
    A = require_gpu()
    seen, first_info, timed_out = [], threading.Event(), []

    def sink(text):
        seen.append(text)
        first_info.set()
        return False

    mcts, tei = _engine(A, 5, 16, capacity=1 << 22, sink=sink)
    tei.set_info_interval(20)

    def stopper():
        if not first_info.wait(60):
            timed_out.append("no info line within 60 s")
        tei.stop()

    th = threading.Thread(target=stopper)
    th.start()
    lines = tei.line("go infinite")
    th.join()
    assert not timed_out, timed_out
    assert tei.line("stop") == []                                       # the line that tz_tei_stop announced
    assert seen and all(INFO.match(s) for s in seen)
    assert len(lines) == 1 and lines[0].startswith("bestmove "), lines  # with a sink the info lines go to the sink alone
    assert mcts.pool_overflows() == 0
    # the stop was consumed: the next search runs to its own limit
    tei.set_info_interval(HUGE_INTERVAL)
    lines = tei.line("go nodes 64")
    assert len(seen[-1:]) == 1 and int(INFO.match(seen[-1]).group(2)) >= 64 and lines[-1].startswith("bestmove ")


def _build_tei_cli(tmp_path):
    from takzero_amd import _lib

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "tei_cli")
    r = subprocess.run(["g++", "-std=c++17", "-O2", "-pthread", os.path.join(root, "examples", "tei_cli.cpp"), "-I" + os.path.join(root, "include"),
                        "-L" + os.path.dirname(_lib.LIB_PATH), "-ltakzero_hip", "-Wl,-rpath," + os.path.dirname(_lib.LIB_PATH), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return exe


def test_tei_cli_program(tmp_path):
    """examples/tei_cli.cpp: the handshake in order, a wrong HalfKomi, a saved .ot, and a search whose bestmove is the session's"""
    from takzero_amd import ot

    A = require_gpu()
    n, leaves, nodes = 4, 8, 40
    exe = _build_tei_cli(tmp_path)
    args = [exe, "--arch", "test", "--n", str(n), "--blocks", "2", "--leaves", str(leaves), "--node-capacity", "65536"]
    r = subprocess.run(args, input="tei\nsetoption name HalfKomi value 2\nisready\n", capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "only 4 is supported" in r.stderr and r.stdout.splitlines()[-1] == "teiok"
    model = str(tmp_path / "model.ot")
    ot.save_ot(model, _weights(n))
    ref = Restated(A, n, leaves, capacity=65536)
    ref.position(None, ["a1"])
    want = ref.go_nodes(nodes)
    p = subprocess.Popen(args, stdin=subprocess.PIPE, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, bufsize=1)
    guard = threading.Timer(120, p.kill)
    guard.start()
    try:
        p.stdin.write("tei\n")
        p.stdin.flush()
        hello = [p.stdout.readline().rstrip("\n") for _ in range(5)]
        assert hello[0].startswith("id name ") and hello[1].startswith("id author ")
        assert hello[2].startswith("option name model type string") and hello[3] == "option name HalfKomi type combo default 4 var 4"
        assert hello[4] == "teiok"
        p.stdin.write("setoption name HalfKomi value 4\nsetoption name model value %s\nisready\n" % model)
        p.stdin.flush()
        ready = p.stdout.readline().rstrip("\n")
        assert ready == "readyok", (ready, p.stderr.read()[-2000:] if not ready else "")
        p.stdin.write("position startpos moves a1\ngo nodes %d\n" % nodes)
        p.stdin.flush()
        lines = []
        while not lines or not lines[-1].startswith("bestmove"):
            line = p.stdout.readline()
            assert line, ("the program ended or was killed at its time limit", lines, p.stderr.read()[-2000:])
            lines.append(line.rstrip("\n"))
        p.stdin.write("quit\n")                                        # only now: the output above was read up to bestmove
        p.stdin.flush()
        assert p.wait(timeout=60) == 0
    finally:
        guard.cancel()
        if p.poll() is None:
            p.kill()
    infos = [INFO.match(l) for l in lines if l.startswith("info time")]
    assert len(infos) >= 1 and all(infos), lines
    assert (int(infos[-1].group(2)), infos[-1].group(4), lines[-1].split()[1]) == want, (lines, want)
