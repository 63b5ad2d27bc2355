"""What every keyed C-ABI entry point and the two row-update forms refuse, status and fr_last_error() text, and what a status word's bits are reported
as, on the MI355X: tests/key_refusals.py against the `gpu` section of tests/golden/key_refusals.json.  A refusal launches nothing; the launches here
are the clean call behind every refusal and the one-block kernels of the status cases, lists of at most 3 keys on a 1500-row model, and the two
host-fed batches of 256 on a shrunk Model-A that the queued-batch refusals need."""
import pytest

import key_refusals as KR

pytestmark = pytest.mark.gpu


def test_refusals_and_status_texts_keep_their_status_text_and_order(fr, gpu):
    KR.check_refusals(fr, gpu)
