// strip_rules_main.cpp - exercises the host-side rules of the STRIP driver (csrc/strip_rules.h) on the CPU; built with
// -fsanitize=address,undefined by tests/test_strip_rules_cpu.py.  Exit status 0: every check held.
#include "strip_rules.h"

#include <cstdio>
#include <vector>

using namespace ttsweep;

static int failures = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) { fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); failures++; } \
    } while (0)

int main()
{
    // ---- are the caller's boxes in step with the padded volumes at the launch?
    float a = 0, b = 0, c = 0;
    std::vector<float *> boxes = {&a, &b, &c};
    CHECK(user_boxes_in_step(true, true, true, true, boxes.data(), 3));       // fresh boxes, batched initialisation
    CHECK(user_boxes_in_step(true, true, false, false, boxes.data(), 3));     // boxes with values: just packed
    CHECK(!user_boxes_in_step(true, true, true, false, boxes.data(), 3));     // fresh boxes, a launch per start
    CHECK(!user_boxes_in_step(false, true, true, true, boxes.data(), 3));     // not the STRIP kernel
    CHECK(!user_boxes_in_step(true, false, true, true, boxes.data(), 3));     // the lanes do not run along z
    CHECK(!user_boxes_in_step(true, false, false, false, boxes.data(), 3));
    CHECK(!user_boxes_in_step(true, true, false, false, nullptr, 3));
    CHECK(!user_boxes_in_step(true, true, false, false, boxes.data(), 0));
    for (size_t hole = 0; hole < boxes.size(); hole++) {                // a start without a box
        std::vector<float *> some = boxes;
        some[hole] = nullptr;
        CHECK(!user_boxes_in_step(true, true, true, true, some.data(), 3));
        CHECK(user_boxes_in_step(true, true, true, true, some.data(), (int)hole) == (hole > 0));
    }
    // ---- may the copy back be left out?  Only in one of the eight cases.
    for (int m = 0; m < 8; m++) {
        const bool in_step = m & 1, at_rest = m & 2, fell_back = m & 4;
        CHECK(unpack_can_be_skipped(in_step, at_rest, fell_back) == (m == 3));
    }
    if (failures) fprintf(stderr, "%d check(s) failed\n", failures);
    else printf("strip rules ok\n");
    return failures ? 1 : 0;
}
