"""lime_amd -- MI355X-native engine for LIME's genomic set-theory hot path.

Intersection, merge (union), subtract (difference), complement, depth of
coverage and the per-row annotation of one set by another (hits, covered
bases, overlap) over ReferenceRegion-keyed interval sets, as hand-written HIP
kernels for gfx950 behind the C-ABI in include/lime_amd.h.  See DESIGN.md.
"""
from ._ffi import LimeError, SUBTRACT_LIME, SUBTRACT_SET, load  # noqa: F401
from .engine import (Annotation, Context, IntervalSet, PAIR_DTYPE, Pairs, Result,  # noqa: F401
                     Space, java_string_order, read_bed)

__version__ = "0.1.0"
