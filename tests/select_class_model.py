"""The model of ss_reads_select_class / `--extract_class` on top of tests/class_model.py: which records a clade holds.

A clade is named by a node: clade 0 is the class 0 alone (the unclassified records); clade c >= 1 is the classes that are c or
lie below c in the forest -- the reads that read_classes.tsv's reads_clade counts for c.  A record of class 0 is in no clade but
clade 0.  An empty record has no class and is in none.
"""
from tests import class_model as cm, rs_model


def in_clade(parent, cls, c):
    """whether class `cls` lies in clade `c`"""
    if c == 0 or cls == 0:
        return c == 0 and cls == 0
    return c in cm.root_path(parent, cls)


def records_of(text):
    """the non-empty records of a flat text, in rs_model.record_ids' numbering"""
    recs = [r for r in bytes(text).split(b"\n") if r]
    assert len(recs) == rs_model.record_ids(text)[1]
    return recs


def selected(text, classes, parent, c):
    """-> the sorted list of the non-empty records of `text` whose class (classes[i] of record i) is in clade c"""
    recs = records_of(text)
    assert len(recs) == len(classes)
    return sorted(r for r, cls in zip(recs, classes) if in_clade(parent, int(cls), c))
