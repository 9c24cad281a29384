"""Which round-key slot a schedule writes (KeySlotPolicy, csrc/aesw_keyring.h): the part of the scheduled key's ring that makes no
HIP call, compiled alone with g++ (no ROCm include, no GPU) and replayed against a restatement of its rules:

  * the ring holds at most "key_slots" slots; a schedule that finds it shorter appends a slot and writes it, one that finds it
    full writes the slot behind the one written last;
  * a ring longer than "key_slots" first sheds its tail, last entry first, into the spare list;
  * a slot that is needed comes from the spare list, newest first, skipping (and dropping) pinned ones, and is a fresh slot only
    when no spare is left;
  * a ring entry a capture has pinned is replaced in place when its turn comes; a pinned slot is never chosen;
  * a schedule whose key launch fails moves the position one back and leaves ring and spares as the step made them.

Every step compares the chosen slot AND the whole state (position, ring, spares) with the model; properties that do not depend on
the model (never a pinned slot, ring within its size, a full turn visits "key_slots" distinct slots, a failed write is chosen
again) are asserted next to it."""
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent


class Model:
    def __init__(self):
        self.pinned, self.ring, self.spare, self.pos, self.size = [], [], [], 0, 4

    def fresh(self):
        self.pinned.append(False)
        return len(self.pinned) - 1

    def take(self):
        while self.spare:
            i = self.spare.pop()
            if not self.pinned[i]:
                return i
        return self.fresh()

    def write(self):
        while len(self.ring) > self.size:
            self.spare.append(self.ring.pop())
        if len(self.ring) < self.size:
            self.ring.append(self.take())
            self.pos = len(self.ring) - 1
        else:
            self.pos = (self.pos + 1) % len(self.ring)
            if self.pinned[self.ring[self.pos]]:
                self.ring[self.pos] = self.take()
        return self.ring[self.pos]

    def run(self, cmd):
        """One command of the driver's script; the line the driver must answer with."""
        slot = None
        op, arg = cmd[0], int(cmd[1:] or 0)
        if op == "i":
            self.spare.append(self.fresh())
        elif op == "s":
            self.size = arg
        elif op == "p":
            self.pinned[arg] = True
        elif op == "c":
            slot = self.fresh()
            self.pinned[slot] = True
        elif op in "wf":
            slot = self.write()
            if op == "f":
                self.pos = (self.pos - 1) % len(self.ring)
        return slot


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = tmp_path_factory.mktemp("keyring") / "keyring_policy_driver"
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I", str(ROOT / "halo2-aes_amd" / "csrc"),
                    str(ROOT / "tests" / "keyring_policy_driver.cpp"), "-o", str(exe)], check=True)

    def run(script):
        text = " ".join(c[0] + (" " + c[1:] if c[1:] else "") for c in script)
        out = subprocess.run([str(exe)], input=text, capture_output=True, text=True, check=True).stdout.splitlines()
        assert len(out) == len(script)
        return out
    return run


def replay(driver, script):
    """Runs the script through the driver and the model; returns the slots the w / f / c commands chose."""
    m, chosen = Model(), []
    for n, (cmd, line) in enumerate(zip(script, driver(script))):
        pinned_before = list(m.pinned)
        slot = m.run(cmd)
        head, spare = line.split("|")
        got = head.split()
        where = (n, cmd, script[:n + 1])
        assert got[0] == ("-" if slot is None else str(slot)), where
        assert int(got[1]) == m.pos and [int(v) for v in got[2:]] == m.ring and [int(v) for v in spare.split()] == m.spare, where
        if cmd[0] in "wf":
            assert not (slot < len(pinned_before) and pinned_before[slot]), where  # never a slot a capture has pinned
            assert len(m.ring) <= m.size and len(set(m.ring)) == len(m.ring) and not set(m.ring) & set(m.spare), where
        if slot is not None:
            chosen.append(slot)
    return chosen


@pytest.mark.parametrize("size", [1, 4, 7])
def test_ring_of_every_size_cycles(driver, size):
    got = replay(driver, ["i", "s%d" % size] + ["w"] * (3 * size + 2))
    assert got[:size] == list(range(size))  # the context's first slot, then fresh ones
    assert got == [i % size for i in range(3 * size + 2)]


def test_shrink_7_to_2_and_grow_back(driver):
    got = replay(driver, ["i", "s7"] + ["w"] * 9 + ["s2"] + ["w"] * 5 + ["s7"] + ["w"] * 12)
    assert got[:9] == [0, 1, 2, 3, 4, 5, 6, 0, 1]
    # the tail goes to the spares; the position (1) stays inside the shorter ring and moves on
    assert got[9:14] == [0, 1, 0, 1, 0]
    # growing back: the spares return newest first (they left last entry first: 6 5 4 3 2), no fresh slot is made
    assert got[14:19] == [2, 3, 4, 5, 6]
    assert got[19:] == [0, 1, 2, 3, 4, 5, 6]
    assert max(got) == 6


def test_shrink_below_the_position(driver):
    got = replay(driver, ["i", "s7"] + ["w"] * 6 + ["s2", "w", "w", "w"])  # position 5 of 7, then a ring of 2
    assert got[6:] == [0, 1, 0]  # (5 + 1) % 2


def test_pins_in_the_middle_of_the_ring(driver):
    # a captured launch pins slots 1 and 2 of a full ring of 4: their ring entries are replaced when their turn comes
    got = replay(driver, ["i", "s4", "w", "w", "w", "w", "p1", "p2"] + ["w"] * 8)
    assert got[4:] == [0, 4, 5, 3, 0, 4, 5, 3]
    # a captured schedule takes a fresh slot of its own in between: the ring's replacement is the one after it
    got = replay(driver, ["i", "s4", "w", "w", "w", "w", "p1", "c", "w", "w", "w"])
    assert got[4:] == [4, 0, 5, 2]


def test_pinned_spares_are_dropped(driver):
    # 7 -> 2 parks 6 5 4 3 2; 5 and 3 are pinned while parked; growing to 5 takes 2, 4, 6 and never 3 or 5; the next one is fresh
    got = replay(driver, ["i", "s7"] + ["w"] * 7 + ["s2", "w", "p5", "p3", "s5", "w", "w", "w", "s6", "w", "w"])
    assert got[7:] == [1, 2, 4, 6, 7, 0]  # (6 + 1) % 2 first
    # the pinned slot is the ring's own current entry, replaced from the spares
    got = replay(driver, ["i", "s3", "w", "w", "w", "s2", "w", "p1", "w", "w", "w"])
    assert got[3:] == [1, 0, 2, 0]  # (2 + 1) % 2, then slot 1's turn comes with slot 1 pinned


FAILS = {
    # a failed write after each kind of step: the slot comes up again (`again`: schedules until it does)
    "first-slot-from-the-spares": (["i", "s4", "f"], 4),
    "growth-with-a-fresh-slot": (["i", "s4", "w", "f"], 4),
    "plain-advance": (["i", "s4", "w", "w", "w", "w", "w", "f"], 1),
    "advance-at-the-wrap": (["i", "s4", "w", "w", "w", "w", "w", "w", "w", "f"], 1),
    "ring-of-one": (["i", "s1", "w", "w", "f"], 1),
    "ring-of-one-first-write": (["i", "s1", "f"], 1),
    "replacement-of-a-pinned-entry-fresh": (["i", "s4", "w", "w", "w", "w", "p1", "w", "f"], 1),
    "replacement-of-a-pinned-entry-from-spares": (["i", "s3", "w", "w", "w", "s2", "w", "p1", "w", "f"], 1),
    "shrink": (["i", "s7"] + ["w"] * 9 + ["s2", "f"], 1),
    "growth-from-the-spares": (["i", "s7"] + ["w"] * 9 + ["s2", "w", "s7", "f"], 7),
    "after-a-captured-schedule": (["i", "s4", "w", "w", "c", "f"], 4),
}


@pytest.mark.parametrize("name", sorted(FAILS))
def test_failed_write_after_each_kind_of_step(driver, name):
    script, again = FAILS[name]
    got = replay(driver, script + ["w"] * (again + 8))
    failed = got[len([c for c in script if c[0] in "wfc"]) - 1]
    after = got[len([c for c in script if c[0] in "wfc"]):]
    # a failure while the ring was still growing leaves the slot in the ring and goes on growing: it comes up after a full turn;
    # in a full ring the very next schedule takes it
    assert after.index(failed) == again - 1, (name, failed, after)


def test_two_failures_in_a_row(driver):
    got = replay(driver, ["i", "s4", "w", "w", "w", "w", "w", "f", "f", "w", "w"])
    assert got[5:] == [1, 1, 1, 2]
