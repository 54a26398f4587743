"""The batched public-key encryption's surface, checked without a GPU: the library exports both entry points, the
binding has both methods (and the timer id of its launches), the public header declares both."""
import re
from pathlib import Path

REPO = Path(__file__).resolve().parents[1]
SYMBOLS = ("fhs_encrypt_asymmetric_batch", "fhs_encode_encrypt_asymmetric_batch")


def test_library_exports_both_symbols():
    import pyPhantom as ph
    for name in SYMBOLS:
        fn = getattr(ph._lib, name)              # AttributeError: the built library lacks it
        assert fn.argtypes is not None and len(fn.argtypes) == (5 if name == SYMBOLS[0] else 9), name


def test_binding_has_both_methods_and_the_timer_id():
    import pyPhantom as ph
    assert callable(ph.public_key.encrypt_asymmetric_batch)
    assert callable(ph.public_key.encode_encrypt_batch)
    assert ph.KERNEL_IDS["encrypt_pk"] == 10
    assert sorted(ph.KERNEL_IDS.values()) == list(range(11))


def test_header_declares_both():
    text = (REPO / "include" / "fhespear.h").read_text()
    for name in SYMBOLS:
        assert re.search(r"fhs_status\s+%s\s*\(\s*fhs_context\s*\*\s*ctx,\s*fhs_public_key\s*\*\s*pk," % name, text), name
    assert "10 encrypt_pk" in text
