"""The text layer of the engine session (csrc/tz_tei.cpp) without a device: tz_tei_parse against Input::from_str
(tei/src/protocol.rs:74-160) and tz_tei_format_info against Output::Info's Display (:240-274).  The expected values are written by
hand from that file: kinds and numbers per input form, one case per ParseInputError, and whole info lines.

The arithmetic behind the info lines, in f32 as the reference does it:
  Value(+-0.005): 0.005f * 100 rounds to 0.5f and 0.005f * 500 to 2.5f exactly, and f32::round takes halves away from zero:
                  cp +-1, wdl 503 0 497 / 497 0 503;
  Win(1), Win(2), Loss(3): f32::from = 0.997, 0.997^2 = 0.994009, -0.997^3 = -0.991027: cp 100, 99, -99; mate ceil(ply / 2)."""
import numpy as np
import pytest

import takzero_amd.api as A
from takzero_amd import _lib

L = _lib
N = 5


def consts():
    import os
    import re

    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "takzero_hip.h")).read()
    return {k: int(v.strip("()")) for k, v in re.findall(r"#define (TZ_TEI_\w+) (\(?-?\d+\)?)", text)}


K = consts()


def parse_error(line, n=N):
    """(TZ_TEI_ERR_* of a line that must not parse, the error text)"""
    import ctypes as C

    lib = _lib.load()
    kind, n_moves = C.c_int(99), C.c_int(0)
    numbers = np.zeros(8, np.int64)
    moves = np.zeros(64, np.uint16)
    text = C.create_string_buffer(256)
    rc = lib.tz_tei_parse(line.encode(), n, C.byref(kind), numbers.ctypes.data, moves.ctypes.data, len(moves), C.byref(n_moves), text, len(text))
    assert rc == -2 and kind.value == K["TZ_TEI_ERROR"], (line, rc, kind.value)      # TZ_EPARSE
    return int(numbers[0]), lib.tz_last_error().decode()


def test_the_constants_are_the_ones_the_cases_below_name():
    assert [K["TZ_TEI_" + k] for k in ("TEI", "ISREADY", "SETOPTION", "NEWGAME", "POSITION", "GO", "STOP", "QUIT")] == list(range(8))
    assert [K["TZ_TEI_GO_" + k] for k in ("WTIME", "BTIME", "WINC", "BINC", "MOVETIME", "NODES", "INFINITE")] == list(range(7))


@pytest.mark.parametrize("line, kind", [("tei", 0), ("isready", 1), ("  stop  ", 6), ("quit", 7), ("isready trailing words", 1)])
def test_single_word_inputs(line, kind):
    k, numbers, moves, text = A.tei_parse(line, N)
    assert k == kind and len(moves) == 0 and text == "" and not numbers.any()


def test_setoption_and_teinewgame():
    k, _, _, text = A.tei_parse("setoption name model value /tmp/model.ot", N)
    assert k == K["TZ_TEI_SETOPTION"] and text == "model /tmp/model.ot"
    k, _, _, text = A.tei_parse("setoption name HalfKomi value 4 ignored", N)
    assert k == K["TZ_TEI_SETOPTION"] and text == "HalfKomi 4"
    k, numbers, _, _ = A.tei_parse("teinewgame 6", N)
    assert k == K["TZ_TEI_NEWGAME"] and numbers[0] == 6


def test_position_forms():
    k, numbers, moves, text = A.tei_parse("position startpos", N)
    assert k == K["TZ_TEI_POSITION"] and numbers[0] == 0 and len(moves) == 0 and text == ""
    k, numbers, moves, text = A.tei_parse("position startpos moves a1 e5 Cc3 Sb2 3c3>12 c3+", N)
    assert k == K["TZ_TEI_POSITION"] and numbers[0] == 0
    assert list(moves) == [A.move_from_ptn(N, m) for m in ("a1", "e5", "Cc3", "Sb2", "3c3>12", "c3+")]
    k, numbers, moves, text = A.tei_parse("position tps x5/x5/x2,12C,x2/x5/2,x3,1 2 3 moves c3< a5", N)
    assert k == K["TZ_TEI_POSITION"] and numbers[0] == 1 and text == "x5/x5/x2,12C,x2/x5/2,x3,1 2 3"
    assert list(moves) == [A.move_from_ptn(N, "c3<"), A.move_from_ptn(N, "a5")]
    k, numbers, moves, text = A.tei_parse("position tps x5/x5/x5/x5/x5 1 1", N)
    assert k == K["TZ_TEI_POSITION"] and numbers[0] == 1 and text == "x5/x5/x5/x5/x5 1 1" and len(moves) == 0
    # protocol.rs:118: anything but `moves` after the position ends the line without moves
    k, _, moves, _ = A.tei_parse("position startpos move a1", N)
    assert k == K["TZ_TEI_POSITION"] and len(moves) == 0
    # the board size is the caller's: the same words on 3x3
    k, _, moves, _ = A.tei_parse("position startpos moves a1 c3", 3)
    assert list(moves) == [A.move_from_ptn(3, "a1"), A.move_from_ptn(3, "c3")]


def test_go_forms():
    k, numbers, _, _ = A.tei_parse("go", N)
    assert k == K["TZ_TEI_GO"] and not numbers.any()
    k, numbers, _, _ = A.tei_parse("go wtime 60000 btime 59000 winc 1000 binc 2000", N)
    assert k == K["TZ_TEI_GO"] and list(numbers) == [0b0001111, 60000, 59000, 1000, 2000, 0, 0, 0]
    k, numbers, _, _ = A.tei_parse("go nodes 12345 movetime 2000", N)
    assert list(numbers) == [0b0110000, 0, 0, 0, 0, 2000, 12345, 0]
    k, numbers, _, _ = A.tei_parse("go infinite", N)
    assert list(numbers) == [0b1000000, 0, 0, 0, 0, 0, 0, 0]
    k, numbers, _, _ = A.tei_parse("go nodes 5 nodes 7 infinite", N)               # the last of a repeated option holds
    assert list(numbers) == [0b1100000, 0, 0, 0, 0, 0, 7, 0]


@pytest.mark.parametrize("line, err, words", [
    ("", "MISSING_FIRST_WORD", "missing first word"),
    ("   \t ", "MISSING_FIRST_WORD", "missing first word"),
    ("hello", "UNRECOGNIZED", "unrecognized option"),
    ("setoption", "MISSING_NAME", "missing `name`"),
    ("setoption model", "MISSING_NAME", "missing `name`"),
    ("setoption name", "MISSING_NAME", "missing `name`"),
    ("setoption name model", "MISSING_VALUE", "missing `value`"),
    ("setoption name model path", "MISSING_VALUE", "missing `value`"),
    ("setoption name model value", "MISSING_NAME", "missing `name`"),            # protocol.rs:97 names MissingName here
    ("teinewgame", "MISSING_SIZE", "missing size after `newgame`"),
    ("teinewgame five", "PARSE_INT", "new game size parse error"),
    ("teinewgame -5", "PARSE_INT", "new game size parse error"),
    ("position", "MISSING_POSITION", "missing second word after `position`"),
    ("position fen", "UNRECOGNIZED", "unrecognized option"),
    ("position tps", "MISSING_TPS", "missing TPS after `position tps`"),
    ("position tps x5/x5/x5/x5/x5 1", "MISSING_TPS", "missing TPS after `position tps`"),
    ("position tps x5/x5/x5/x5 1 1", "PARSE_TPS", "position tps parse error"),    # four ranks
    ("position tps x5/x5/x5/x5/x4,7 1 1", "PARSE_TPS", "position tps parse error"),
    ("position tps x5/x5/x5/x5/x5 3 1", "PARSE_TPS", "position tps parse error"),
    ("position startpos moves a1 z9", "PARSE_MOVE", "move parse error"),
    ("position startpos moves a1 2a1", "PARSE_MOVE", "move parse error"),          # a count on a placement
    ("go wtime", "MISSING_SECONDS", "missing seconds after time parameter in `go`"),
    ("go nodes 10 movetime", "MISSING_SECONDS", "missing seconds after time parameter in `go`"),
    ("go nodes", "MISSING_AMOUNT", "missing the amount of nodes after `go nodes`"),
    ("go nodes many", "PARSE_INT", "parse error"),
    ("go movetime 1.5", "PARSE_INT", "parse error"),
    ("go depth 5", "UNRECOGNIZED", "unrecognized option"),
])
def test_every_parse_error(line, err, words):
    code, text = parse_error(line)
    assert code == K["TZ_TEI_ERR_" + err], (line, code, text)
    assert words in text, (line, text)


def test_parse_checks_its_buffers():
    import ctypes as C

    lib = _lib.load()
    kind, n_moves = C.c_int(0), C.c_int(0)
    numbers = np.zeros(8, np.int64)
    moves = np.zeros(2, np.uint16)
    text = C.create_string_buffer(8)
    rc = lib.tz_tei_parse(b"position startpos moves a1 b1 c1", N, C.byref(kind), numbers.ctypes.data, moves.ctypes.data, 2, C.byref(n_moves), text, 8)
    assert rc == -1 and n_moves.value == 3                                          # TZ_EINVAL, and how many there are
    rc = lib.tz_tei_parse(b"position tps x5/x5/x5/x5/x5 1 1", N, C.byref(kind), numbers.ctypes.data, moves.ctypes.data, 2, C.byref(n_moves), text, 8)
    assert rc == -1


def f32_bits(x):
    return int(np.float32(x).view(np.uint32))


PV = ("a1", "Cb2", "Sc3", "3c3>12")


def info(time_ms, nodes, tag, bits, pv=PV):
    return A.tei_format_info(N, time_ms, nodes, tag, bits, [A.move_from_ptn(N, m) for m in pv])


def test_info_value_scores_round_halves_away_from_zero():
    assert info(1000, 2000, A.EVAL_VALUE, f32_bits(0.005)) == "info time 1000 nodes 2000 nps 2000 wdl 503 0 497 score cp 1 pv a1 Cb2 Sc3 3c3>12"
    assert info(1000, 2000, A.EVAL_VALUE, f32_bits(-0.005)) == "info time 1000 nodes 2000 nps 2000 wdl 497 0 503 score cp -1 pv a1 Cb2 Sc3 3c3>12"
    assert info(300, 128, A.EVAL_VALUE, f32_bits(0.25), ("a1",)) == "info time 300 nodes 128 nps 426 wdl 625 0 375 score cp 25 pv a1"


def test_info_wdl_at_the_ends_of_the_value_range():
    assert info(7, 3, A.EVAL_VALUE, f32_bits(-1.0), ()) == "info time 7 nodes 3 nps 428 wdl 0 0 1000 score cp -100 pv"
    assert info(7, 3, A.EVAL_VALUE, f32_bits(0.0), ()) == "info time 7 nodes 3 nps 428 wdl 500 0 500 score cp 0 pv"
    assert info(7, 3, A.EVAL_VALUE, f32_bits(1.0), ()) == "info time 7 nodes 3 nps 428 wdl 1000 0 0 score cp 100 pv"


def test_info_solved_scores():
    assert info(10, 50, A.EVAL_WIN, 1, ("a1",)) == "info time 10 nodes 50 nps 5000 wdl 1000 0 0 score mate 1 score cp 100 pv a1"
    assert info(10, 50, A.EVAL_WIN, 2, ("a1", "b1")) == "info time 10 nodes 50 nps 5000 wdl 1000 0 0 score mate 1 score cp 99 pv a1 b1"
    assert info(10, 50, A.EVAL_LOSS, 3, ("a1", "b1", "c1")) == "info time 10 nodes 50 nps 5000 wdl 0 0 1000 score mate -2 score cp -99 pv a1 b1 c1"
    assert info(10, 50, A.EVAL_DRAW, 4, ("a1",)) == "info time 10 nodes 50 nps 5000 wdl 0 1000 0 score cp 0 pv a1"


def test_info_with_an_empty_pv_and_at_zero_milliseconds():
    assert info(250, 0, A.EVAL_VALUE, f32_bits(0.5), ()) == "info time 250 nodes 0 nps 0 wdl 750 0 250 score cp 50 pv"
    assert info(0, 128, A.EVAL_VALUE, f32_bits(0.5), ("e5",)) == "info time 0 nodes 128 nps 0 wdl 750 0 250 score cp 50 pv e5"     # the reference divides by zero


def test_format_info_checks_its_arguments():
    import ctypes as C

    lib = _lib.load()
    out = C.create_string_buffer(16)
    assert lib.tz_tei_format_info(N, 1, 1, 0, 0, None, 0, out, 16) == -1            # too small for any info line
    assert lib.tz_tei_format_info(N, 1, 1, 9, 0, None, 0, out, 16) == -1            # no such Eval
    big = C.create_string_buffer(256)
    n = lib.tz_tei_format_info(N, 1, 1, 0, 0, None, 0, big, 256)
    assert n == len(big.value) == len("info time 1 nodes 1 nps 1000 wdl 500 0 500 score cp 0 pv")
