"""The shapes tests/test_session_class_edges_gpu.py runs sfa_session_classes on, as data, and what the two kernels of
sigfish_amd/csrc/sdtw_session_class.hpp do at a shape -- derived from the documented layout alone, not from the library:
  * a slot's row is total_columns floats; the rows of a session lie back to back behind a pad of 256 words on a 16-byte boundary,
    so slot s begins (s * total_columns) mod 4 words behind a 16-byte boundary
  * the head are the columns in front of the row's first 16-byte boundary (the whole row if it ends before that), the body whole
    quads of 4 columns, the tail what is left; head and tail columns are taken by part 0, lanes 0.. and 64..
  * a block has 256 threads and is handed a part of 2048 quads; thread t offers quads part * 2048 + t + 256 * u, u = 0 .. 7
  * a row has class_parts = max(ceil((total_columns / 4) / 2048), 1) parts (total / 4 rounded down), whatever its head
  * a quad at column g takes its four mask bits from words g >> 5 and (g >> 5) + 1 shifted by g & 31: shifts 29, 30, 31 straddle
tests/test_class_shapes_cpu.py asserts what the GPU file's cases claim to reach, without a GPU."""
from collections import namedtuple

THREADS = 256
QUADS_PER_LANE = 8
PART_QUADS = THREADS * QUADS_PER_LANE
PART_COLUMNS = 4 * PART_QUADS

Shape = namedtuple("Shape", "name rna lens n_slots")  # rna: RNA | INV, one strand; otherwise DNA, two strands


def total_columns(shape):
    return sum(shape.lens) * (1 if shape.rna else 2)


# rows at every alignment: one strand, so that the total can be odd.  (offset of a row, total) modulo 4: see reachable_pairs
SMALL = [Shape("rna_465", True, [37, 64, 65, 299], 9),   # = 1 (mod 4): offsets 0, 1, 2, 3 as the slot number runs
         Shape("rna_466", True, [37, 64, 65, 300], 9),   # = 2: offsets 0, 2
         Shape("rna_467", True, [37, 64, 65, 301], 9),   # = 3: offsets 0, 3, 2, 1
         Shape("rna_468", True, [37, 64, 65, 302], 9),   # = 0: offset 0
         Shape("dna_930", False, [37, 64, 65, 299], 9)]  # = 2, two strands

# rows shorter than two quads: a head that is the whole row, no body, a tail without a body
TINY = [Shape(f"rna_{n}", True, [n], 5) for n in (1, 2, 3, 5, 6, 7)]

WIDE = [Shape("rna_16385", True, [8193, 8192], 5),           # slot 0 (and 4): two exactly full parts; the others 4095 quads
        Shape("rna_8197", True, [8197], 5),                  # two parts; slot 1 (head 3): 2048 quads, part 1 offers nothing
        Shape("rna_16433", True, [4099, 4097, 8201, 36], 5),  # three parts, the last with 12 quads
        Shape("dna_20006", False, [4097, 4096, 1810], 5)]    # three parts, a contig (both strands) inside each

HUGE = Shape("rna_524301", True, [524301], 5)  # 65 parts: the rows kernel's second round of 64

# the reference [A, A] and a contig of one k-mer behind it that makes the total odd, so that the rows begin at every alignment:
# column j and column |A| + j of a row are equal; see seat() for where the twin sits
TIES = [Shape(f"ties_{n}", True, [n, n, 1], 5) for n in (4, 256, 1024, 8192)]

INF = Shape("rna_inf", True, [37, 64, 65, 299], 5)  # contig 2's levels are 3e38
SPREAD = Shape("rna_467_spread", True, [37, 64, 65, 301], 9)

Layout = namedtuple("Layout", "offset head nq tail parts part_quads shifts")


def class_parts(total):
    return max((total // 4 + PART_QUADS - 1) // PART_QUADS, 1)


def layout(total, slot):
    """Layout of slot `slot` of a session whose rows have `total` columns:
    offset      words between the last 16-byte boundary and the row's column 0
    head, tail  columns taken one by one in front of and behind the body
    nq          quads of the body
    parts       blocks of the slot
    part_quads  [parts] quads each part has to offer (0: the part offers nothing)
    shifts      set of the mask shifts g & 31 of the body's quads"""
    offset = (slot * total) % 4
    head = min((4 - offset) % 4, total)
    nq = (total - head) // 4
    tail = total - head - 4 * nq
    parts = class_parts(total)
    part_quads = [min(max(nq - p * PART_QUADS, 0), PART_QUADS) for p in range(parts)]
    shifts = {(head + 4 * q) % 32 for q in range(min(nq, 8))}
    return Layout(offset, head, nq, tail, parts, part_quads, shifts)


def us_of(n_quads):
    """the u of a part that offers n_quads quads at which some lane has a column"""
    return {u for u in range(QUADS_PER_LANE) if n_quads > u * THREADS}


def waves_of(n_quads):
    """the waves of such a block whose lanes have a body column (the others hand on `nothing met`)"""
    return {w for w in range(THREADS // 64) if n_quads > 64 * w}


def seat(total, slot, col):
    """Who offers column `col` of the slot's row: ('head', lane), ('tail', lane) or ('body', part, u, wave, lane of the wave)"""
    lay = layout(total, slot)
    assert 0 <= col < total
    if col < lay.head:
        return ("head", col)
    if col >= lay.head + 4 * lay.nq:
        return ("tail", 64 + col - lay.head - 4 * lay.nq)
    part, r = divmod((col - lay.head) // 4, PART_QUADS)
    u, t = divmod(r, THREADS)
    return ("body", part, u, t // 64, t % 64)


def reachable_pairs():
    """(row offset, total) modulo 4 that exist at all: the offset is slot * total modulo 4, so an even total never gives an odd one"""
    return {((s * t) % 4, t) for s in range(4) for t in range(4)}


def part_interior(total, part):
    """[lo, hi): columns that belong to `part` whatever the slot's head is (0 .. 3) and that are body columns for every slot"""
    lo = part * PART_COLUMNS + 3
    hi = min((part + 1) * PART_COLUMNS, total - 3)  # (a body ends at total - ((total - head) mod 4) >= total - 3)
    return lo, hi
