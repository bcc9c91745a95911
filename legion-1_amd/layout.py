"""The layout of a batch's two counter arrays, nc and ec: include/legion_batch_layout.h in Python.

Same names (without the C prefix), same functions, over anything indexable -- a list, a NumPy array, a ctypes array, a tensor.
The header draws the layout word by word; this module only restates it.  Pure Python: no ctypes, no NumPy, no torch, so a
consumer that reads the counters by its own means can still use it.
"""
MAX_HOPS = 5
COUNTER_WORDS = 16          # int32 words of nc and of ec
LEVEL_WORDS = 2             # nc words per level: (offset, size), level after level from word 3
COUNTER_BYTES = 4 * COUNTER_WORDS

# the fixed words
NC_TOTAL = 0                # running node total
NC_HOP_NEW = 1              # new nodes of the hop in flight
NC_NEXT_INPUTS = 2          # input slots of the next hop
EC_TOTAL = 0                # running edge total
EC_HOP = 1                  # edges of the hop in flight
EC_INPUT_OFF = 2            # offset of the current hop's input list in agg_src_ids (scratch, not a total)

assert 5 + LEVEL_WORDS * MAX_HOPS < COUNTER_WORDS and 2 + MAX_HOPS < COUNTER_WORDS


# ---- word indices ----
def idx_level_offset(l):
    return 3 + LEVEL_WORDS * l


def idx_level_size(l):
    return 4 + LEVEL_WORDS * l


def idx_nodes_through(l):
    return 5 + LEVEL_WORDS * l


def idx_edges_through(h):
    return 2 + h


def idx_level(offset_word):
    """Inverse of idx_level_offset."""
    return (offset_word - 3) // LEVEL_WORDS


# ---- nodes ----
def level_offset(nc, l):
    return int(nc[idx_level_offset(l)])


def level_size(nc, l):
    return int(nc[idx_level_size(l)])


def nodes_through(nc, l):
    return int(nc[idx_nodes_through(l)])


def batch_nodes(nc, H):
    """Nodes of an H-hop batch: the length of ids and the rows of the features."""
    return nodes_through(nc, H)


def first_block_dst(nc, H):
    """n_in: the nodes of the levels < H."""
    return level_offset(nc, H)


# ---- edges ----
def edges_through(ec, h):
    """Edges of the hops 1..h; 0 for h < 1 (word 2 is scratch)."""
    return 0 if h < 1 else int(ec[idx_edges_through(h)])


def hop_edges_begin(ec, h):
    return edges_through(ec, h - 1)


def hop_edges_end(ec, h):
    return edges_through(ec, h)


def batch_edges(ec, H):
    return edges_through(ec, H)


# ---- both ----
def hop_inputs(nc, ec, h):
    """Input slots of hop h: the seeds at h = 1, else one per edge of hop h - 1."""
    return level_size(nc, 0) if h == 1 else hop_edges_end(ec, h - 1) - hop_edges_begin(ec, h - 1)


def agg_rows(nc, ec, H):
    """Rows of the feature buffer an aggregated batch fills: the levels < H, then one row of sums per input slot of hop H."""
    return first_block_dst(nc, H) + hop_inputs(nc, ec, H)
