// Host check of csrc/walk_shape.h (tests/test_walk_shape_cpu.py builds it with the address and undefined-behaviour
// sanitizers as a stand-alone program): which shapes take a shaped instantiation of the walk and which the generic one.
#include "walk_shape.h"

#include <initializer_list>
#include <stdio.h>

using ivfhnsw_gpu_impl::walk_shape_for;
using ivfhnsw_gpu_impl::WalkShape;

static int failures = 0;

static void expect(const char *what, WalkShape got, int d, int maxM)
{
    if (got.d != d || got.maxM != maxM) {
        printf("%s: got (%d, %d), want (%d, %d)\n", what, got.d, got.maxM, d, maxM);
        failures++;
    }
}

int main()
{
    // the cases of tests/test_gpu_walk_shape.py: d 128 / maxM 32 at ef 40, 33 (nch 1) and 80 (nch 2), both filter forms
    for (int nch = 1; nch <= 2; nch++)
        for (int fmode = 2; fmode <= 3; fmode++)
            for (int tagw : {8, 10, 12, 16}) {
                expect("d 128, maxM 32", walk_shape_for(128, 32, 32, fmode, tagw, nch, true), 128, 32);
                expect("d 96 (DEEP)", walk_shape_for(96, 32, 32, fmode, tagw, nch, true), 96, 32);
                expect("the knob at 0", walk_shape_for(128, 32, 32, fmode, tagw, nch, false), 0, 0);
                expect("maxM 16", walk_shape_for(128, 16, 32, fmode, tagw, nch, true), 0, 0);
                expect("d 64", walk_shape_for(64, 32, 32, fmode, tagw, nch, true), 0, 0);
                expect("maxM 64", walk_shape_for(128, 64, 64, fmode, tagw, nch, true), 0, 0);
                expect("a record of 64 rows", walk_shape_for(128, 32, 64, fmode, tagw, nch, true), 0, 0);
                expect("d 112", walk_shape_for(112, 32, 32, fmode, tagw, nch, true), 0, 0);
            }
    // forms that have no shaped instantiation: no filter, the gather form, the global bitmap, larger result sets
    expect("fmode 0", walk_shape_for(128, 32, 32, 0, 10, 2, true), 0, 0);
    expect("fmode 1", walk_shape_for(128, 32, 32, 1, 10, 2, true), 0, 0);
    expect("bitmap only", walk_shape_for(128, 32, 32, 2, 0, 2, true), 0, 0);
    for (int nch : {3, 4, 8, 16})
        expect("nch > 2", walk_shape_for(128, 32, 32, 3, 10, nch, true), 0, 0);
    expect("nch 0", walk_shape_for(128, 32, 32, 3, 10, 0, true), 0, 0);
    // the bench's graphs: 993 127 and 2^17 nodes, d 128, maxM 32, ef 80 and 100
    expect("1B", walk_shape_for(128, 32, 32, 3, 10, 2, true), 128, 32);
    expect("100M", walk_shape_for(128, 32, 32, 2, 8, 2, true), 128, 32);
    if (failures) {
        printf("walk_shape: %d checks failed\n", failures);
        return 1;
    }
    printf("walk_shape ok\n");
    return 0;
}
