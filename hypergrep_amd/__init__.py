"""MI355X-native multi-pattern line scanner with the hypergrep Python API (drop-in for `import hypergrep`)."""

from hypergrep_amd.utils import (  # the reference package re-exports exactly these names
    CALLBACK_TYPE,
    HS_EXT_FLAG_EDIT_DISTANCE,
    HS_EXT_FLAG_HAMMING_DISTANCE,
    HS_EXT_FLAG_MAX_OFFSET,
    HS_EXT_FLAG_MIN_LENGTH,
    HS_EXT_FLAG_MIN_OFFSET,
    HS_FLAG_CASELESS,
    HS_FLAG_DOTALL,
    HS_FLAG_MULTILINE,
    HS_FLAG_SINGLEMATCH,
    RC_INVALID_FILE,
    ExprExt,
    Result,
    check_compatibility,
    configure_libraries,
    count,
    count_files,
    count_values,
    count_values_files,
    count_values_top,
    grep,
    grep_files,
    prepare_patterns,
    scan,
    scan_files,
)

__all__ = [
    "CALLBACK_TYPE", "HS_FLAG_CASELESS", "HS_FLAG_DOTALL", "HS_FLAG_MULTILINE", "HS_FLAG_SINGLEMATCH", "RC_INVALID_FILE", "Result",
    "check_compatibility", "configure_libraries", "grep", "prepare_patterns", "scan",
    # extended parameters (approximate matching), beyond the reference's names
    "ExprExt", "HS_EXT_FLAG_MIN_OFFSET", "HS_EXT_FLAG_MAX_OFFSET", "HS_EXT_FLAG_MIN_LENGTH", "HS_EXT_FLAG_EDIT_DISTANCE",
    "HS_EXT_FLAG_HAMMING_DISTANCE",
    # many files in one native call
    "grep_files", "scan_files",
    # counts per report id, taken on the GPU
    "count", "count_files",
    # distinct matched parts and their counts, grouped on the GPU
    "count_values",
    # ... for many files in one native call, ranked by count and cut to the most frequent of every file on the GPU
    "count_values_files",
    # ... for one file of any number of chunks, accumulated in a value store on the GPU and cut to the most frequent there
    "count_values_top",
]
__version__ = "0.1.0"
