"""The report decoders of api.py on the CPU: check_report_dict (7 words), circ_report_dict (8) and cols_report_dict (12) on int64
tensors, and the CheckReport structure path of last_stream_check / check_witness_host.  The expected dicts were produced once by the
decoders as they stood before they were given one shared core (commit 3fecb7c), on these very vectors; a device writes the
report as uint64, torch hands it over as int64, so `first = none` (and `first_cell = none`) arrives as -1."""
import pytest
import torch

# (name, the twelve words, check_report_dict(words[:7]), circ_report_dict(words[:8]), cols_report_dict(words))
CASES = [
    ('clean', [5, 2, 0, 0, 0, 0, -1, 0, 0, 0, -1, 1234],
     {'blocks': 5, 'keys': 2, 'lookup_failures': 0, 'copy_failures': 0, 'gate_failures': 0, 'input_failures': 0, 'first': None, 'satisfied': True},
     {'blocks': 5, 'keys': 2, 'lookup_failures': 0, 'copy_failures': 0, 'gate_failures': 0, 'input_failures': 0, 'first': None, 'offset_failures': 0, 'satisfied': True},
     {'blocks': 5, 'keys': 2, 'lookup_failures': 0, 'copy_failures': 0, 'gate_failures': 0, 'input_failures': 0, 'first': None, 'offset_failures': 0, 'satisfied': True, 'cell_failures': 0, 'unassigned_failures': 0, 'first_cell': None, 'cells': 1234}),
    ('first_packed', [5, 2, 3, 0, 0, 0, 78187970287, 0, 0, 0, -1, 1234],
     {'blocks': 5, 'keys': 2, 'lookup_failures': 3, 'copy_failures': 0, 'gate_failures': 0, 'input_failures': 0, 'first': (74565, True, 5, 48879), 'satisfied': False},
     {'blocks': 5, 'keys': 2, 'lookup_failures': 3, 'copy_failures': 0, 'gate_failures': 0, 'input_failures': 0, 'first': (74565, True, 5, 48879), 'offset_failures': 0, 'satisfied': False},
     {'blocks': 5, 'keys': 2, 'lookup_failures': 3, 'copy_failures': 0, 'gate_failures': 0, 'input_failures': 0, 'first': (74565, True, 5, 48879), 'offset_failures': 0, 'satisfied': False, 'cell_failures': 0, 'unassigned_failures': 0, 'first_cell': None, 'cells': 1234}),
    ('lookup', [5, 2, 9, 0, 0, 0, -1, 0, 0, 0, -1, 1234],
     {'blocks': 5, 'keys': 2, 'lookup_failures': 9, 'copy_failures': 0, 'gate_failures': 0, 'input_failures': 0, 'first': None, 'satisfied': False},
     {'blocks': 5, 'keys': 2, 'lookup_failures': 9, 'copy_failures': 0, 'gate_failures': 0, 'input_failures': 0, 'first': None, 'offset_failures': 0, 'satisfied': False},
     {'blocks': 5, 'keys': 2, 'lookup_failures': 9, 'copy_failures': 0, 'gate_failures': 0, 'input_failures': 0, 'first': None, 'offset_failures': 0, 'satisfied': False, 'cell_failures': 0, 'unassigned_failures': 0, 'first_cell': None, 'cells': 1234}),
    ('copy', [5, 2, 0, 10, 0, 0, -1, 0, 0, 0, -1, 1234],
     {'blocks': 5, 'keys': 2, 'lookup_failures': 0, 'copy_failures': 10, 'gate_failures': 0, 'input_failures': 0, 'first': None, 'satisfied': False},
     {'blocks': 5, 'keys': 2, 'lookup_failures': 0, 'copy_failures': 10, 'gate_failures': 0, 'input_failures': 0, 'first': None, 'offset_failures': 0, 'satisfied': False},
     {'blocks': 5, 'keys': 2, 'lookup_failures': 0, 'copy_failures': 10, 'gate_failures': 0, 'input_failures': 0, 'first': None, 'offset_failures': 0, 'satisfied': False, 'cell_failures': 0, 'unassigned_failures': 0, 'first_cell': None, 'cells': 1234}),
    ('gate', [5, 2, 0, 0, 11, 0, -1, 0, 0, 0, -1, 1234],
     {'blocks': 5, 'keys': 2, 'lookup_failures': 0, 'copy_failures': 0, 'gate_failures': 11, 'input_failures': 0, 'first': None, 'satisfied': False},
     {'blocks': 5, 'keys': 2, 'lookup_failures': 0, 'copy_failures': 0, 'gate_failures': 11, 'input_failures': 0, 'first': None, 'offset_failures': 0, 'satisfied': False},
     {'blocks': 5, 'keys': 2, 'lookup_failures': 0, 'copy_failures': 0, 'gate_failures': 11, 'input_failures': 0, 'first': None, 'offset_failures': 0, 'satisfied': False, 'cell_failures': 0, 'unassigned_failures': 0, 'first_cell': None, 'cells': 1234}),
    ('input', [5, 2, 0, 0, 0, 12, -1, 0, 0, 0, -1, 1234],
     {'blocks': 5, 'keys': 2, 'lookup_failures': 0, 'copy_failures': 0, 'gate_failures': 0, 'input_failures': 12, 'first': None, 'satisfied': False},
     {'blocks': 5, 'keys': 2, 'lookup_failures': 0, 'copy_failures': 0, 'gate_failures': 0, 'input_failures': 12, 'first': None, 'offset_failures': 0, 'satisfied': False},
     {'blocks': 5, 'keys': 2, 'lookup_failures': 0, 'copy_failures': 0, 'gate_failures': 0, 'input_failures': 12, 'first': None, 'offset_failures': 0, 'satisfied': False, 'cell_failures': 0, 'unassigned_failures': 0, 'first_cell': None, 'cells': 1234}),
    ('offset', [5, 2, 0, 0, 0, 0, -1, 14, 0, 0, -1, 1234],
     {'blocks': 5, 'keys': 2, 'lookup_failures': 0, 'copy_failures': 0, 'gate_failures': 0, 'input_failures': 0, 'first': None, 'satisfied': True},
     {'blocks': 5, 'keys': 2, 'lookup_failures': 0, 'copy_failures': 0, 'gate_failures': 0, 'input_failures': 0, 'first': None, 'offset_failures': 14, 'satisfied': False},
     {'blocks': 5, 'keys': 2, 'lookup_failures': 0, 'copy_failures': 0, 'gate_failures': 0, 'input_failures': 0, 'first': None, 'offset_failures': 14, 'satisfied': False, 'cell_failures': 0, 'unassigned_failures': 0, 'first_cell': None, 'cells': 1234}),
    ('cell', [5, 2, 0, 0, 0, 0, -1, 0, 15, 0, -1, 1234],
     {'blocks': 5, 'keys': 2, 'lookup_failures': 0, 'copy_failures': 0, 'gate_failures': 0, 'input_failures': 0, 'first': None, 'satisfied': True},
     {'blocks': 5, 'keys': 2, 'lookup_failures': 0, 'copy_failures': 0, 'gate_failures': 0, 'input_failures': 0, 'first': None, 'offset_failures': 0, 'satisfied': True},
     {'blocks': 5, 'keys': 2, 'lookup_failures': 0, 'copy_failures': 0, 'gate_failures': 0, 'input_failures': 0, 'first': None, 'offset_failures': 0, 'satisfied': False, 'cell_failures': 15, 'unassigned_failures': 0, 'first_cell': None, 'cells': 1234}),
    ('unassigned', [5, 2, 0, 0, 0, 0, -1, 0, 0, 16, -1, 1234],
     {'blocks': 5, 'keys': 2, 'lookup_failures': 0, 'copy_failures': 0, 'gate_failures': 0, 'input_failures': 0, 'first': None, 'satisfied': True},
     {'blocks': 5, 'keys': 2, 'lookup_failures': 0, 'copy_failures': 0, 'gate_failures': 0, 'input_failures': 0, 'first': None, 'offset_failures': 0, 'satisfied': True},
     {'blocks': 5, 'keys': 2, 'lookup_failures': 0, 'copy_failures': 0, 'gate_failures': 0, 'input_failures': 0, 'first': None, 'offset_failures': 0, 'satisfied': False, 'cell_failures': 0, 'unassigned_failures': 16, 'first_cell': None, 'cells': 1234}),
    ('first_cell', [5, 2, 0, 0, 0, 0, -1, 0, 0, 0, 17, 1234],
     {'blocks': 5, 'keys': 2, 'lookup_failures': 0, 'copy_failures': 0, 'gate_failures': 0, 'input_failures': 0, 'first': None, 'satisfied': True},
     {'blocks': 5, 'keys': 2, 'lookup_failures': 0, 'copy_failures': 0, 'gate_failures': 0, 'input_failures': 0, 'first': None, 'offset_failures': 0, 'satisfied': True},
     {'blocks': 5, 'keys': 2, 'lookup_failures': 0, 'copy_failures': 0, 'gate_failures': 0, 'input_failures': 0, 'first': None, 'offset_failures': 0, 'satisfied': True, 'cell_failures': 0, 'unassigned_failures': 0, 'first_cell': 17, 'cells': 1234}),
    ('cells', [5, 2, 0, 0, 0, 0, -1, 0, 0, 0, -1, 18],
     {'blocks': 5, 'keys': 2, 'lookup_failures': 0, 'copy_failures': 0, 'gate_failures': 0, 'input_failures': 0, 'first': None, 'satisfied': True},
     {'blocks': 5, 'keys': 2, 'lookup_failures': 0, 'copy_failures': 0, 'gate_failures': 0, 'input_failures': 0, 'first': None, 'offset_failures': 0, 'satisfied': True},
     {'blocks': 5, 'keys': 2, 'lookup_failures': 0, 'copy_failures': 0, 'gate_failures': 0, 'input_failures': 0, 'first': None, 'offset_failures': 0, 'satisfied': True, 'cell_failures': 0, 'unassigned_failures': 0, 'first_cell': None, 'cells': 18}),
    ('negative', [-3, 2, 0, 0, 0, -9223372036854775808, -2, 0, 0, 0, -2, 1234],
     {'blocks': 18446744073709551613, 'keys': 2, 'lookup_failures': 0, 'copy_failures': 0, 'gate_failures': 0, 'input_failures': 9223372036854775808, 'first': (17592186044415, True, 7, 65534), 'satisfied': False},
     {'blocks': 18446744073709551613, 'keys': 2, 'lookup_failures': 0, 'copy_failures': 0, 'gate_failures': 0, 'input_failures': 9223372036854775808, 'first': (17592186044415, True, 7, 65534), 'offset_failures': 0, 'satisfied': False},
     {'blocks': 18446744073709551613, 'keys': 2, 'lookup_failures': 0, 'copy_failures': 0, 'gate_failures': 0, 'input_failures': 9223372036854775808, 'first': (17592186044415, True, 7, 65534), 'offset_failures': 0, 'satisfied': False, 'cell_failures': 0, 'unassigned_failures': 0, 'first_cell': 18446744073709551614, 'cells': 1234}),
]


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_the_three_decoders(pkg, case):
    _name, words, check, circ, cols = case
    t = torch.tensor(words, dtype=torch.int64)
    assert pkg.api.check_report_dict(t[:7]) == check
    assert pkg.api.circ_report_dict(t[:8]) == circ
    assert pkg.api.cols_report_dict(t) == cols
    # a decoder reads the words it knows and ignores what follows them
    assert pkg.api.check_report_dict(t[:8]) == check and pkg.api.check_report_dict(t) == check
    assert pkg.api.circ_report_dict(t) == circ


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_the_structure_path_gives_the_same_dict(pkg, case):
    _name, words, check, _circ, _cols = case
    rep = pkg.api.CheckReport()
    for (field, _type), w in zip(pkg.api.CheckReport._fields_, words):
        setattr(rep, field, w & 0xFFFFFFFFFFFFFFFF)
    assert pkg.api._decode_struct(rep) == check  # what last_stream_check and check_witness_host return
