"""CPU tier: the ground the STRIP schedule tests (test_gpu_strip_schedules.py) stand on, checked where no GPU is:
the host-side mirror of the layout rule against the grids, the star, the starts and the groups of SCHEDULES."""
import numpy as np

import strip_cases as S


def test_layouts_have_neighbours_on_every_axis():
    """A change of STRIP_K, STRIP_TB or the layout rule that leaves the main grid with one lane tile, one strip,
    whole remainders or an even plane count fails here."""
    main, second = S.check_layouts()
    assert main.units(1) == 650 and main.units(2) == 330 and second.units(1) == 165


def test_star_reaches_seven_cells_and_is_asymmetric(pkg):
    offs = S.star_offsets()
    assert S.check_star(offs) > 0
    flags = [e[3] for e in pkg.build_pull_star(pkg.inputs.make_fs(offs))]
    assert flags.count(1) > 0 and flags.count(1) == flags.count(2)      # forward-only / reverse-only pull entries


def test_starts_and_schedule_groups():
    S.check_schedule_groups()
    m = S.StripLayout(S.MAIN_SHAPE)
    st = S.main_starts()
    assert st.shape == (11, 3) and (st >= 0).all() and (st < np.array(S.MAIN_SHAPE)).all()
    assert st[3][m.bax] >= (m.btiles - 1) * m.TB and st[4][m.cax] >= (m.cstrips - 1) * m.K
    assert st[5][m.aax] == m.planes - 1 and (st[6] == st[3]).all()
    sec = S.second_starts()
    assert (sec >= 0).all() and (sec < np.array(S.SECOND_SHAPE)).all()
    for one_launch, options in S.SCHEDULES:
        assert one_launch in (0, 1) and all(k.startswith("OPT_") for k in options)
