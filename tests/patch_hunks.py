"""rust/halo2-aes-patch/aesw-witness.patch read hunk by hunk, and what the tests pin about the upstream files it applies to
(test infrastructure: tests/test_rust_shim.py checks, tests/golden/make_golden.py writes tests/golden/patch_upstream.json).

A hunk applies with `patch -p1 --fuzz=0` and no offset exactly when lines old_start .. old_start + old_lines - 1 of the
upstream file are its old side (its context and '-' lines): the golden file keeps the SHA-256 digest of those upstream
lines, never the lines.  COUNTS are single-line patterns, so a file's count is the sum over its lines, and the patched
file's count is the upstream count minus the '-' lines' count plus the '+' lines' count."""
import hashlib
import re

HEADER = re.compile(r"^@@ -(\d+)(?:,(\d+))? \+(\d+)(?:,(\d+))? @@")

# name -> single-line regular expression counted in the chip files
COUNTS = {
    "xor_bytes": re.escape("xor_bytes"),
    "z_at": re.escape("aesw::z_at(at)"),
    "copy_advice": re.escape("copy_advice("),
    "value_closure": r"\|\| (?:crate::)?aesw::[xyz]_at\(at\)",
    "advance_1": r"let at = (?:crate::)?aesw::advance\(1\);",
}
CHIP_FILES = ["src/chips/u8_xor_chip.rs", "src/chips/sbox_chip.rs", "src/chips/gf_mul_chip.rs"]


def parse(text):
    """[(file, old_start, old_lines, new_start, new_lines, body)]; body = the hunk's lines as written, tag first.  A hunk's
    body ends when both sides hold as many lines as its header says."""
    lines = text.splitlines()
    hunks, path, i = [], None, 0
    while i < len(lines):
        if lines[i].startswith("+++ b/"):
            path = lines[i][6:]
        elif lines[i].startswith("@@"):
            m = HEADER.match(lines[i])
            if not m:
                raise ValueError("line %d: bad hunk header %r" % (i + 1, lines[i]))
            a, b, c, d = int(m.group(1)), int(m.group(2) or 1), int(m.group(3)), int(m.group(4) or 1)
            body, old, new = [], 0, 0
            i += 1
            while i < len(lines) and (old < b or new < d):
                tag = lines[i][:1]
                if tag not in (" ", "-", "+"):
                    raise ValueError("line %d: %r inside a hunk of %s" % (i + 1, lines[i], path))
                old += tag != "+"
                new += tag != "-"
                body.append(lines[i])
                i += 1
            hunks.append((path, a, b, c, d, body))
            continue
        i += 1
    return hunks


def old_side(body):
    return [l[1:] for l in body if l[:1] in (" ", "-")]


def new_side(body):
    return [l[1:] for l in body if l[:1] in (" ", "+")]


def digest(lines):
    return hashlib.sha256("\n".join(lines).encode()).hexdigest()


def counts(lines):
    return {name: sum(len(re.findall(rx, l)) for l in lines) for name, rx in COUNTS.items()}
