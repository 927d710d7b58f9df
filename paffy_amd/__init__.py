"""paffy_amd -- MI355X (gfx950) implementation of paffy's per-record PAF/CIGAR hot path.

The product is the C-ABI library `libpaffy_hip.so` (include/paffy_hip.h); this package is the
Python host mirror used by the tests and bench.py. There is no CPU fallback: importing the
engine without the built library, or without a GPU, raises.
"""
from .engine import (ADD_MISMATCHES, DECHUNK, FILTER, INVERT, PASS, REMOVE_MISMATCHES, SHATTER, STATS, TRIM_ENDS, TRIM_FIXED, TRIM_IDENTITY, UPCONVERT, Engine,
                     PafError, PlanInfo, Stage, add_mismatches, build_library, chain, dechunk, dedupe, filter, invert, library_path, pipe, shatter, split_file, stage,
                     stage_dechunk, stage_trim_ends, tile, trim, upconvert, view, view_stats)
from . import shard  # noqa: E402,F401 -- paffy_amd.shard.tile_sharded / chain_sharded: the commands sharded by query sequence

__all__ = ["Engine", "Stage", "PlanInfo", "PafError", "stage", "stage_trim_ends", "stage_dechunk", "pipe", "invert", "shatter", "trim", "add_mismatches", "tile", "chain", "filter", "dedupe", "split_file",
           "dechunk", "upconvert", "view", "view_stats", "build_library", "library_path", "shard",
           "INVERT", "TRIM_IDENTITY", "TRIM_FIXED", "SHATTER", "ADD_MISMATCHES", "REMOVE_MISMATCHES", "PASS", "FILTER", "TRIM_ENDS", "STATS", "DECHUNK", "UPCONVERT"]
