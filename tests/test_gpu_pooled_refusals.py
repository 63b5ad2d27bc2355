"""What every pooled C-ABI entry point refuses, status and fr_last_error() text, on the MI355X: tests/pooled_refusals.py against the `gpu` section of
tests/golden/pooled_refusals.json (the sharded pair: two shard contexts of the one device on the staged host exchange).  A refusal launches nothing;
the launches here are the clean call behind every refusal, batch 16 on a 2000-row model."""
import pytest

import pooled_refusals as PR

pytestmark = pytest.mark.gpu


def test_refusals_keep_their_status_text_and_order(fr, gpu):
    PR.check_refusals(fr, gpu)
