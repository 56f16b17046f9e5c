"""rwkv.cpp_amd -- MI355X-native drop-in for the rwkv.cpp hot path (librwkv.so + its Python host mirror).

The directory name contains a dot, so import it through `__graft_entry__.load_package()` (importlib by path) or add the
repo root to sys.path and use `importlib.import_module("rwkv.cpp_amd")` is NOT possible; see __graft_entry__.py.
"""
from .rwkv_cpp import (  # noqa: F401
    BeamParams,
    CUT_HOOKS_LIB_PATH,
    CutParams,
    DECAY_HOOKS_LIB_PATH,
    DRAFT_MAX,
    GUIDE_HOOKS_LIB_PATH,
    GUIDE_MAX,
    GUIDE_MAX_STATES,
    HOOKS_LIB_PATH,
    LIB_PATH,
    NO_GUIDE,
    NO_TARGET,
    NO_TOKEN,
    PenaltyParams,
    RepParams,
    RWKVBatch,
    RWKVContext,
    RWKVModel,
    RWKVSharedLibrary,
    SAMPLE_HOOKS_LIB_PATH,
    SampleParams,
    StopParams,
    TOP_MAX,
    build_library,
    guide_edges,
    load_rwkv_shared_library,
    lookup_draft,
    penalty_params,
    sample_params,
    stop_params,
)
