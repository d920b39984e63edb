"""alevin-fry_amd — MI355X-native `alevin-fry quant` hot path.

The directory name carries a hyphen (it mirrors the reference's name), so import it
with `importlib.import_module("alevin-fry_amd")`.  Contents:
  csrc/       hand-written HIP kernels for gfx950 + the C ABI of include/afquant.h
  afquant.py  host-side mirror of the reference's per-cell quant interface (ctypes)
  rad.py      collated-RAD chunk codec (host)
  synth.py    seeded synthetic inputs
"""
from . import _abi, rad, synth  # noqa: F401
from .afquant import AfqError, Quantifier, QuantResult, WorkerConfig, atac_collate, atac_collate_limits, atac_generate_permit_list, atac_gpl_limits, atac_sort_limits, atac_sort_table_slot, collate, collate_limits, collate_multi, collate_multi_limits, convert, convert_limits, convert_prelude, generate_permit_list_multi, gpl_limits, gpl_multi_limits, gpl_table_slot, inflate_limits, load_library, snappy_decode_limits, snappy_limits, view  # noqa: F401
