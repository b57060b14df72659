"""MI355OPT_WORDS16 as a new context parses it (context.hip config_from_env through mi_debug_words16_option; no GPU): on
when unset, off at 0, on at any other integer, and -- an integer-valued option like MAX_GRID -- a value that is no integer
is ignored with a warning and the default stays."""
import pytest

from optimization_amd import capi


def test_words16_is_on_unless_switched_off(capfd):
    assert capi.words16_option(None) is True
    assert capi.words16_option("0") is False
    assert capi.words16_option("1") is True
    assert capi.words16_option("0x0") is False and capi.words16_option("2") is True   # (strtol, base 0)
    assert "warning" not in capfd.readouterr().err


@pytest.mark.parametrize("text", ["", "yes", "off", "no", "false", "1.5", "0 "])
def test_words16_takes_integers_only(capfd, text):
    assert capi.words16_option(text) is True   # the default stays
    err = capfd.readouterr().err
    assert f'warning: MI355OPT_WORDS16="{text}" is not an integer; ignored' in err
