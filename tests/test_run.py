"""The run of one circuit's blocks (csrc/aesw_run.h: how both accumulators cut [first_block, first_block + n_blocks) at the set
boundaries into pieces and every piece into chunks, the grid the host plans for it and the chunk a workgroup finds in it).
The header is compiled alone with g++ -- no ROCm include, no GPU -- into tests/run_driver.cpp, which sweeps, for every K in
9 ... 14 with 1 ... 4 sets, every (first_block, n_blocks >= 1) with first_block + n_blocks <= capacity under chunks 1, 2, 5, 17
and the default:

  * the host plan (set0, pieces, longest piece, pairs) against a count that places every block of the run with
    Placement::locate (itself held against the reference's rule by tests/test_placement.py);
  * the kernels' side, Run::chunk_at, evaluated at every (x, y) of the planned grid: every chunk lies in its set and in the
    run, and the chunks cover each block of the run exactly once per half;
  * run_default_chunk on the shapes and values tests/test_acc_library.py pins, and the 2^22 bound on the pairs of a set."""
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
CASES = [(k, n_sets) for k in range(9, 15) for n_sets in range(1, 5)]


def capacity(k, n_sets):
    """The reference's rule (tests/test_placement.py): set 0 gives up 1760 rows, every set holds whole 1360-row blocks."""
    return max((1 << k) - 1760, 0) // 1360 + (n_sets - 1) * ((1 << k) // 1360)


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = tmp_path_factory.mktemp("run") / "run_driver"
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I", str(ROOT / "halo2-aes_amd" / "csrc"),
                    str(ROOT / "tests" / "run_driver.cpp"), "-o", str(exe)], check=True)

    def ask(commands):
        text = "\n".join(" ".join(str(v) for v in c) for c in commands)
        done = subprocess.run([str(exe)], input=text, capture_output=True, text=True, check=True)
        out = done.stdout.splitlines()
        assert len(out) == len(commands), done.stderr
        return [[int(v) for v in line.split()] for line in out], done.stderr
    return ask


def test_plan_and_chunks_against_a_walk_over_every_block(driver):
    answers, complaints = driver([("s", k, n_sets) for k, n_sets in CASES])
    for (k, n_sets), (cap, cases, failures) in zip(CASES, answers):
        assert cap == capacity(k, n_sets), (k, n_sets)
        assert cases == 5 * cap * (cap + 1) // 2, (k, n_sets)  # every (first, n >= 1) that fits, five chunks each
        assert failures == 0, (k, n_sets, complaints)
    assert complaints == ""
    assert sum(cases for _cap, cases, _f in answers) > 10000 and capacity(14, 4) == 46 and capacity(10, 4) == 0 and capacity(11, 4) == 3


def test_the_longest_piece_is_the_first_the_last_or_a_whole_set_between(driver):
    """The shapes of the shortcut, by hand at K = 14 / N = 3 (10 + 12 + 12 blocks): set0, pieces, longest, pairs, chunk, fits."""
    asked = [(0, 34, 5), (8, 16, 5), (9, 2, 1), (3, 4, 17), (8, 26, 5), (9, 14, 5), (22, 12, 0), (0, 34, 0)]
    want = [[0, 3, 12, 3, 5, 1],    # three whole sets
            [0, 3, 12, 3, 5, 1],    # 2 / 12 / 2: the middle piece is the longest (acc_cases.RAGGED's add (8, 16))
            [0, 2, 1, 1, 1, 1],     # one block on either side of a boundary
            [0, 1, 4, 1, 17, 1],    # inside one set
            [0, 3, 12, 3, 5, 1],    # 2 / 12 / 12: the last piece as long as the whole set between
            [0, 3, 12, 3, 5, 1],    # 1 / 12 / 1
            [2, 1, 12, 1, 256, 1],  # the last set alone, the default chunk
            [0, 3, 12, 1, 256, 1]]
    answers, _ = driver([("p", 14, 3, first, n, chunk) for first, n, chunk in asked])
    assert answers == want


def test_the_default_chunk_and_the_bound_on_the_pairs_of_a_set(driver):
    cap, big = capacity(24, 4), capacity(30, 1024)
    assert cap == 49342
    asked = [34, 1, 3083, cap, 1 << 15, cap - (1 << 15), big, 0, 100, 40000, 1 << 22]
    answers, _ = driver([("d", n) for n in asked])
    got = dict(zip(asked, (a[0] for a in answers)))
    # what tests/test_acc_library.py pins through the built library: the floor of 256, 128 pairs above it
    assert got[34] == got[1] == got[3083] == got[1 << 15] == got[cap - (1 << 15)] == got[0] == got[100] == 256
    assert got[cap] == 386 and got[big] == -(-big // 128) and got[40000] == -(-40000 // 128) and got[1 << 22] == 1 << 15
    # more than 2^22 chunks in one set do not fit the grid: one set at K = 40, one block per pair
    answers, _ = driver([("p", 40, 1, 0, 1 << 22, 1), ("p", 40, 1, 5, (1 << 22) + 1, 1), ("p", 40, 1, 5, (1 << 22) + 1, 2)])
    assert answers == [[0, 1, 1 << 22, 1 << 22, 1, 1], [0, 1, (1 << 22) + 1, (1 << 22) + 1, 1, 0], [0, 1, (1 << 22) + 1, (1 << 21) + 1, 2, 1]]
