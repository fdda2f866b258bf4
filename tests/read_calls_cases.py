"""The inputs of the read-call device tests (tests/test_read_calls_gpu.py): class_cases' tables, forest and blocks, and one block of
this file's own with the one record class_cases has none of -- a record with a list entry above 65535, which 16 bits per kept
node could not hold.  tests/test_read_calls_host.py checks on the model that every case the device test is about is there.
"""
from tests import class_cases as cc

REPEAT_NODE = 151      # the node of stretch 150
REPEATS = 3000


def repeat_record(g):
    """200 bases of one stretch 3000 times over: 600 kb, one node; even the table that lists every 7th k-mer finds 24 of its
    k-mers in every copy, 72 000 hits"""
    s = (REPEAT_NODE - 1) * cc.STRETCH
    return g[s:s + 200] * REPEATS


def repeat_block(g):
    """a few reads of 150, the repeat record, a few more: the record lies neither first nor last"""
    lines = cc.one_length_block(g).split(b"\n")[:-1]
    return b"".join(r + b"\n" for r in lines[:40] + [repeat_record(g)] + lines[40:52])


def blocks(g):
    """name -> flat block: what the device test classifies as file-order ASCII sets"""
    out = {"ragged_%d" % t: cc.ragged_block(g, t) for t in (0, 1, 1023)}
    out["one_length"] = cc.one_length_block(g)
    out["repeat"] = repeat_block(g)
    return out
