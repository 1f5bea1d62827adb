"""CPU tier: the life cycle of a handle under the emulation library (lifecycle_cases.py) -- a refused finalize leaves a handle that can be
finalized again or closed, and tsnet_stage_ptr("src_fea") reports the images of the kind of forward that ran last."""
import lifecycle_cases as lc


def test_failed_finalize_then_retry(emu_lib):
    lc.failed_finalize_then_retry(emu_lib, "cpu")


def test_src_fea_count_by_kind(emu_lib):
    lc.src_fea_count_by_kind(emu_lib, "cpu")


def test_destroy_without_finalize(emu_lib):
    cfg, sd = lc.net()
    lc.new_engine(cfg, emu_lib, "cpu").close()              # never finalized
    lc.refused(cfg, sd, emu_lib, "cpu").close()             # finalize refused
