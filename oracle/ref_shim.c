/* ref_shim.c -- calls the REFERENCE's own compiled primitives through the oracle's argument types.
 * TEST INFRASTRUCTURE ONLY (see zng_oracle.h).
 *
 * This file is our own text; it is compiled only by oracle/Makefile (target ref-prims), against the reference's
 * headers and with exactly the definitions of the cmake build whose libz-ng.a it is linked with (taken from that
 * build's compile_commands.json: deflate_state's layout depends on them).  The result, oracle/_ref/libzng_ref_prims*.so,
 * is never committed.
 *
 * Every ref_* function mirrors the oracle_* function of the same name in zng_oracle.h.  A call that takes a state
 * copies the oracle_deflate_state into a zeroed reference deflate_state (the slabs are shared, not copied), binds
 * s->update_hash the way lm_init does (deflate.c:1223-1234: rolling when max_chain_length > 1024), calls the
 * reference function, and copies match_start / ins_h back.
 */
#include <string.h>

#include "zbuild.h"
#include "deflate.h"
#include "arch/generic/generic_functions.h"

#include "zng_oracle.h"

#define REF_EXPORT __attribute__((visibility("default")))

static void to_ref(deflate_state *s, const oracle_deflate_state *o) {
    memset(s, 0, sizeof(*s));
    s->window = o->window;
    s->prev = o->prev;
    s->head = o->head;
    s->w_size = o->w_size;
    s->w_bits = o->w_bits;
    s->w_mask = o->w_mask;
    s->window_size = o->window_size;
    s->lookahead = o->lookahead;
    s->strstart = o->strstart;
    s->match_start = o->match_start;
    s->prev_length = o->prev_length;
    s->max_chain_length = o->max_chain_length;
    s->good_match = o->good_match;
    s->nice_match = o->nice_match;
    s->level = o->level;
    s->ins_h = o->ins_h;
    if (s->max_chain_length > 1024) {
        s->update_hash = &update_hash_roll;
        s->insert_string = &insert_string_roll;
        s->quick_insert_string = &quick_insert_string_roll;
    } else {
        s->update_hash = &update_hash;
        s->insert_string = &insert_string;
        s->quick_insert_string = &quick_insert_string;
    }
}

static void from_ref(oracle_deflate_state *o, const deflate_state *s) {
    o->match_start = s->match_start;
    o->ins_h = s->ins_h;
}

REF_EXPORT void ref_slide_hash(oracle_deflate_state *o) {
    deflate_state s;
    to_ref(&s, o);
    slide_hash_c(&s);
    from_ref(o, &s);
}

REF_EXPORT uint32_t ref_compare256(const uint8_t *src0, const uint8_t *src1) {
    return compare256_c(src0, src1);
}

REF_EXPORT uint32_t ref_update_hash(uint32_t h, uint32_t val) {
    return update_hash(h, val);
}

REF_EXPORT oracle_pos ref_quick_insert_string(oracle_deflate_state *o, uint32_t str) {
    deflate_state s;
    to_ref(&s, o);
    Pos head = quick_insert_string(&s, str);
    from_ref(o, &s);
    return head;
}

REF_EXPORT void ref_insert_string(oracle_deflate_state *o, uint32_t str, uint32_t count) {
    deflate_state s;
    to_ref(&s, o);
    insert_string(&s, str, count);
    from_ref(o, &s);
}

REF_EXPORT uint32_t ref_update_hash_roll(uint32_t h, uint32_t val) {
    return update_hash_roll(h, val);
}

REF_EXPORT oracle_pos ref_quick_insert_string_roll(oracle_deflate_state *o, uint32_t str) {
    deflate_state s;
    to_ref(&s, o);
    Pos head = quick_insert_string_roll(&s, str);
    from_ref(o, &s);
    return head;
}

REF_EXPORT void ref_insert_string_roll(oracle_deflate_state *o, uint32_t str, uint32_t count) {
    deflate_state s;
    to_ref(&s, o);
    insert_string_roll(&s, str, count);
    from_ref(o, &s);
}

REF_EXPORT uint32_t ref_longest_match(oracle_deflate_state *o, oracle_pos cur_match) {
    deflate_state s;
    to_ref(&s, o);
    uint32_t len = longest_match_c(&s, cur_match);
    from_ref(o, &s);
    return len;
}

REF_EXPORT uint32_t ref_longest_match_slow(oracle_deflate_state *o, oracle_pos cur_match) {
    deflate_state s;
    to_ref(&s, o);
    uint32_t len = longest_match_slow_c(&s, cur_match);
    from_ref(o, &s);
    return len;
}

REF_EXPORT uint32_t ref_chunksize(void) {
    return chunksize_c();
}

REF_EXPORT uint8_t *ref_chunkmemset_safe(uint8_t *out, uint8_t *from, unsigned len, unsigned left) {
    return chunkmemset_safe_c(out, from, len, left);
}

/* which probe form longest_match_c was compiled with in this build (8 = byte pairs, 64 = 8-byte probes) */
REF_EXPORT int ref_optimal_cmp(void) {
    return OPTIMAL_CMP;
}
