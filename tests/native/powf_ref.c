/* Test helper: the host glibc powf the reference's display chain calls
 * (gui.cpp:11-16 through CImg's pow(), main.cpp:225-235), so tests can compare
 * ipt_math.h's powf_ and the display kernels to it bit-for-bit. Built by
 * tests/display_ref.py with gcc -O2 -ffp-contract=off. */
#define _GNU_SOURCE
#include <math.h>
#include <pthread.h>

typedef struct { const float* in; float y; float* out; long lo, hi; } job_t;

static void* run(void* a) {
    job_t* j = (job_t*)a;
    for (long i = j->lo; i < j->hi; ++i) j->out[i] = powf(j->in[i], j->y);
    return 0;
}
void powf_eval(const float* in, float y, float* out, long n, int nthreads) {
    if (nthreads < 1) nthreads = 1;
    if (nthreads > 64) nthreads = 64;
    pthread_t th[64];
    job_t jobs[64];
    for (int t = 0; t < nthreads; ++t) {
        jobs[t].in = in; jobs[t].y = y; jobs[t].out = out;
        jobs[t].lo = n * t / nthreads; jobs[t].hi = n * (t + 1) / nthreads;
        pthread_create(&th[t], 0, run, &jobs[t]);
    }
    for (int t = 0; t < nthreads; ++t) pthread_join(th[t], 0);
}
