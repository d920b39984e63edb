"""The collate judge (tests/collate_judge.py) on vectors derived by hand from the reference's text: the expected bytes are typed out
here, byte for byte.  Widths of one byte (barcode, UMI, position) keep them readable: a head is 6 bytes, an alignment 5."""
import collate_judge as J

# two input chunks.  r1: na 0, barcode 0A.  r2: barcode 1A (corrected to 0A), alignments fw / rc / fw with positions 11 22 33.
# r3: barcode 77 (not in the map), one rc alignment.  r4 (second chunk): barcode 0B, one rc alignment.
R1 = "00000000 0A 01"
R2 = "03000000 1A 02  05000080 11  06000000 22  07000080 33"
R3 = "01000000 77 03  01000000 44"
R4 = "01000000 0B 04  09000000 55"
CHUNK_A = "2E000000 03000000" + R1 + R2 + R3   # 8 + 6 + 21 + 11 = 46 bytes
CHUNK_B = "13000000 01000000" + R4             # 8 + 11 = 19 bytes
DATA = bytes.fromhex(CHUNK_A + CHUNK_B)
OFF = [0, 46]
CORR = {0x0A: 0x0A, 0x1A: 0x0A, 0x0B: 0x0B, 0x0D: 0x0D}
CELLS = [0x0B, 0x0A, 0x0D]   # 0D receives nothing
EMPTY = "08000000 00000000"


def run(ori):
    return J.collate(DATA, OFF, 1, 1, 1, ori, CORR, CELLS)


def test_cells_are_ordered_by_count_descending_then_barcode_ascending():
    assert J.cell_order({0x0B: 2, 0x0D: 1, 0x0A: 2, 0x0C: 5}) == [0x0C, 0x0A, 0x0B, 0x0D]
    assert J.cell_order([(9, 1), (3, 1), (7, 1)]) == [3, 7, 9]


def test_both_keeps_every_alignment_and_the_record_without_one():
    w = run("both")
    cell_b = "13000000 01000000" + R4
    cell_a = "23000000 02000000" + R1 + "03000000 0A 02  05000080 11  06000000 22  07000080 33"   # the corrected barcode, the UMI unchanged
    assert w["bytes"] == bytes.fromhex(cell_b + cell_a + EMPTY)
    assert w["chunk_off"] == [0, 19, 54, 62] and w["nrec"] == [1, 2, 0]
    assert w["stats"] == dict(n_records=4, n_compatible=4, n_uncorrected=1, n_kept=3, n_alignments_in=5, n_alignments_kept=4, n_long_records=0, out_bytes=62)
    assert run("either") == w


def test_rc_drops_two_of_three_alignments_and_the_record_without_one():
    w = run("rc")
    cell_b = "13000000 01000000" + R4
    cell_a = "13000000 01000000  01000000 0A 02  06000000 22"   # na becomes 1; the kept word and ITS position byte
    assert w["bytes"] == bytes.fromhex(cell_b + cell_a + EMPTY)
    assert w["chunk_off"] == [0, 19, 38, 46] and w["nrec"] == [1, 1, 0]
    assert w["stats"] == dict(n_records=4, n_compatible=3, n_uncorrected=1, n_kept=2, n_alignments_in=5, n_alignments_kept=2, n_long_records=0, out_bytes=46)


def test_fw_keeps_bit_31_and_leaves_a_cell_empty():
    w = run("fw")
    cell_a = "18000000 01000000  02000000 0A 02  05000080 11  07000080 33"   # bit 31 stays set in the words
    assert w["bytes"] == bytes.fromhex(EMPTY + cell_a + EMPTY)
    assert w["chunk_off"] == [0, 8, 32, 40] and w["nrec"] == [0, 1, 0]
    # r3 and r4 have no forward alignment: not compatible, so r3's unknown barcode is never looked up
    assert w["stats"] == dict(n_records=4, n_compatible=1, n_uncorrected=0, n_kept=1, n_alignments_in=5, n_alignments_kept=2, n_long_records=0, out_bytes=40)


def test_an_unobserved_barcode_is_dropped_and_counted():
    w = J.collate(DATA, OFF, 1, 1, 1, "both", {0x0B: 0x0B}, [0x0B])
    assert w["nrec"] == [1] and w["stats"]["n_uncorrected"] == 3 and w["stats"]["n_kept"] == 1
    assert w["bytes"] == bytes.fromhex("13000000 01000000" + R4)


def test_input_order_inside_a_cell_is_chunk_then_record():
    data = bytes.fromhex("14000000 02000000  00000000 0A 01  00000000 0B 02" + "14000000 02000000  00000000 0B 03  00000000 0A 04")
    w = J.collate(data, [0, 20], 1, 1, 0, "both", {0x0A: 0x0C, 0x0B: 0x0C}, [0x0C])
    assert w["bytes"] == bytes.fromhex("20000000 04000000" + "00000000 0C 01  00000000 0C 02  00000000 0C 03  00000000 0C 04")


def test_long_record_count_follows_the_limit():
    assert J.collate(DATA, OFF, 1, 1, 1, "both", CORR, CELLS, lane_alns=2)["stats"]["n_long_records"] == 1
    assert J.collate(DATA, OFF, 1, 1, 1, "both", CORR, CELLS, lane_alns=3)["stats"]["n_long_records"] == 0
