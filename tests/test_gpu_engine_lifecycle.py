"""GPU tier: lifecycle_cases.py on the device -- the refused finalize (a host check between packing launches) and its retry, and the image
count of tsnet_stage_ptr("src_fea") after a forward of each kind."""
import pytest

import lifecycle_cases as lc

pytestmark = pytest.mark.gpu


def test_failed_finalize_then_retry():
    lc.failed_finalize_then_retry(None, "cuda")


def test_src_fea_count_by_kind():
    lc.src_fea_count_by_kind(None, "cuda")
