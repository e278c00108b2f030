/* topup_ref.c -- TEST INFRASTRUCTURE: a plain C statement of what
 * mm_blend_pixels computes (include/mm_api.h), IEEE binary32 in the order
 * written there, built with the oracle Makefile's CFLAGS (-ffp-contract=off,
 * no fast-math).  tests/topup_support.py binds it.
 *
 * With -DTOPUP_MAIN it is a stand-alone program (for a sanitizer build): it
 * blends a seeded list, with entries inside and outside the window, into a
 * seeded window and prints a checksum of the result's bits. */
#include <stdint.h>
#include <stdlib.h>

/* image: w*h float4, the window (x0, y0, w, h); pixels: n pairs (x, y);
 * extra: n float4.  Entries in list order (a window pixel named twice ends
 * with the later entry's result on top of the earlier one's).  Returns the
 * number of entries inside the window. */
uint64_t topup_blend(float* image, uint32_t x0, uint32_t y0, uint32_t w, uint32_t h, const uint32_t* pixels,
                     const float* extra, uint64_t n, float m) {
    uint64_t inside = 0;
    for (uint64_t e = 0; e < n; ++e) {
        const uint32_t x = pixels[2 * e], y = pixels[2 * e + 1];
        if (x < x0 || x - x0 >= w || y < y0 || y - y0 >= h) continue;
        float* A = image + 4 * ((size_t)(y - y0) * w + (x - x0));
        const float* E = extra + 4 * e;
        const float Nn = A[3] + m;
        for (int c = 0; c < 3; ++c) A[c] = A[c] + ((E[c] - A[c]) * m) / Nn;
        A[3] = Nn;
        ++inside;
    }
    return inside;
}

#ifdef TOPUP_MAIN
#include <stdio.h>
#include <string.h>

static uint32_t lcg(uint32_t* s) { return *s = *s * 1664525u + 1013904223u; }

int main(void) {
    enum { W = 37, H = 5, X0 = 11, Y0 = 7, N = 300 };
    uint32_t s = 12345u;
    float* image = malloc(sizeof(float) * 4 * W * H);
    uint32_t* pixels = malloc(sizeof(uint32_t) * 2 * N);
    float* extra = malloc(sizeof(float) * 4 * N);
    if (!image || !pixels || !extra) return 2;
    for (int i = 0; i < 4 * W * H; ++i) image[i] = (i & 3) == 3 ? 1.0f + (float)(lcg(&s) >> 28) : (float)(lcg(&s) >> 8) * 0x1p-24f;
    for (int e = 0; e < N; ++e) {
        pixels[2 * e] = lcg(&s) >> 26;  /* 0..63: some left and right of the window */
        pixels[2 * e + 1] = lcg(&s) >> 28;
        for (int c = 0; c < 4; ++c) extra[4 * e + c] = (float)(lcg(&s) >> 8) * 0x1p-24f;
    }
    pixels[0] = 0x80000000u; pixels[1] = 0x80000000u;
    pixels[2] = X0 + W; pixels[3] = Y0;
    pixels[4] = X0; pixels[5] = Y0 + H;
    const uint64_t inside = topup_blend(image, X0, Y0, W, H, pixels, extra, N, 3.0f);
    uint32_t sum = 0;
    for (int i = 0; i < 4 * W * H; ++i) {
        uint32_t b;
        memcpy(&b, &image[i], 4);
        sum = sum * 31u + b;
    }
    printf("inside %llu checksum %08x\n", (unsigned long long)inside, sum);
    free(image); free(pixels); free(extra);
    return inside > 0 && inside < N ? 0 : 1;
}
#endif
