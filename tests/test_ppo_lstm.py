"""CPU: host-side validation of arl_net_set_ppo_state, the LSTM's opt-in to the PPO epochs, and of what
arl_net_set_ppo / arl_net_set_ppo_options accept once it is set -- unbound handles, no kernel launches."""
import ctypes

OK, EINVAL, ESTATE = 0, 1, 3
FAKE = 1 << 40            # 256-byte aligned, never dereferenced
SNAP, CARRY, VOLD, AUX = (FAKE + (k << 30) for k in (1, 2, 3, 4))
LSTM, RGB, STACK, STATES, NATURE = 1, 16, 32, 64, 2


def make(lib, arch):
    h = ctypes.c_void_p()
    assert lib.arl_net_create(ctypes.byref(h), arch, 4, 32, 5, 0, 0) == 0
    return h


def test_the_symbol_is_an_addition_to_abi_4():
    from asyncrl_amd._lib import SIGNATURES, lib
    assert "arl_net_set_ppo_state" in SIGNATURES
    assert lib.arl_abi_version() == 4


def test_set_ppo_state_validation():
    from asyncrl_amd._lib import lib
    for arch, want in ((LSTM, OK), (LSTM | RGB, OK), (0, ESTATE), (RGB, ESTATE), (STACK, ESTATE), (STATES, ESTATE),
                       (NATURE, ESTATE)):
        h = make(lib, arch)
        try:
            assert lib.arl_net_set_ppo_state(h, CARRY) == want, arch
            if want == ESTATE:
                assert b"LSTM" in lib.arl_last_error()
                assert lib.arl_net_set_ppo_state(h, None) == ESTATE, arch
            else:
                assert lib.arl_net_set_ppo_state(h, CARRY + 4) == EINVAL        # 16-byte alignment
                assert lib.arl_net_set_ppo_state(h, CARRY + 8) == EINVAL
                assert lib.arl_net_set_ppo_state(h, None) == OK                 # unset: PPO is off
                assert lib.arl_net_set_ppo_state(h, None) == OK
        finally:
            lib.arl_net_destroy(h)
    assert lib.arl_net_set_ppo_state(None, CARRY) == EINVAL
    assert lib.arl_net_set_ppo_state(None, None) == EINVAL


def test_null_while_ppo_is_set_is_refused():
    from asyncrl_amd._lib import lib
    h = make(lib, LSTM)
    try:
        assert lib.arl_net_set_ppo_state(h, CARRY) == OK
        assert lib.arl_net_set_ppo(h, SNAP, 0.2) == OK
        assert lib.arl_net_set_ppo_state(h, None) == ESTATE and b"off first" in lib.arl_last_error()
        assert lib.arl_net_set_ppo_state(h, CARRY + 16) == OK                   # another buffer: fine while set
        assert lib.arl_net_set_ppo(h, None, 0.0) == OK
        assert lib.arl_net_set_ppo_state(h, None) == OK
    finally:
        lib.arl_net_destroy(h)


def test_the_lstm_takes_ppo_once_it_has_a_carry_buffer():
    from asyncrl_amd._lib import lib
    for arch in (LSTM, LSTM | RGB):
        h = make(lib, arch)
        try:
            # the default: today's refusal, which now also names the way in
            assert lib.arl_net_set_ppo(h, SNAP, 0.2) == ESTATE
            assert b"FF" in lib.arl_last_error() and b"arl_net_set_ppo_state" in lib.arl_last_error()
            assert lib.arl_net_set_ppo_options(h, 1, 0.2, VOLD, AUX) == ESTATE
            assert b"FF" in lib.arl_last_error() and b"arl_net_set_ppo_state" in lib.arl_last_error()
            # with a carry buffer
            assert lib.arl_net_set_ppo_state(h, CARRY) == OK
            assert lib.arl_net_set_ppo(h, SNAP, 0.2) == OK
            assert lib.arl_net_set_ppo_options(h, 1, 0.2, VOLD, AUX) == OK
            assert lib.arl_net_set_ppo_options(h, 0, 0.0, None, AUX) == OK
            for bad in (0.0, 1.0, -0.1, 1.5, float("nan"), float("inf")):
                assert lib.arl_net_set_ppo(h, SNAP, bad) == EINVAL, bad
            assert lib.arl_net_set_ppo(h, SNAP + 4, 0.2) == EINVAL
            assert lib.arl_net_set_ppo_options(h, 0, -1.0, VOLD, AUX) == EINVAL
            assert lib.arl_net_set_ppo_options(h, 0, 0.2, VOLD + 4, AUX) == EINVAL
            assert lib.arl_net_set_ppo_options(h, 1, 0.0, None, AUX + 4) == EINVAL
            assert lib.arl_net_set_ppo_options(h, 1, 0.0, None, None) == EINVAL
            # an unbound handle still launches nothing
            assert lib.arl_ppo_begin(h, 0.99, 1, None) == ESTATE and b"bound" in lib.arl_last_error()
            # off again, carry unset: the old refusal is back
            assert lib.arl_net_set_ppo_options(h, 0, 0.0, None, None) == OK
            assert lib.arl_net_set_ppo(h, None, 0.0) == OK
            assert lib.arl_net_set_ppo_state(h, None) == OK
            assert lib.arl_net_set_ppo(h, SNAP, 0.2) == ESTATE and b"FF" in lib.arl_last_error()
            assert lib.arl_net_set_ppo_options(h, 1, 0.0, None, AUX) == ESTATE and b"FF" in lib.arl_last_error()
        finally:
            lib.arl_net_destroy(h)


def test_the_nature_head_stays_refused():
    from asyncrl_amd._lib import lib
    h = make(lib, NATURE)
    try:
        assert lib.arl_net_set_ppo_state(h, CARRY) == ESTATE
        assert lib.arl_net_set_ppo(h, SNAP, 0.2) == ESTATE and b"FF" in lib.arl_last_error()
    finally:
        lib.arl_net_destroy(h)
