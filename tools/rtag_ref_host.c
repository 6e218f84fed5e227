/* tools/rtag_ref_host.c -- DEVELOPMENT-MACHINE TOOL of tools/gen_rtag_golden.py.  Drives the reference's own filter_rewrite_tag on one
 * chunk and records what it hands to its emitter.  The plugin is compiled where it lies in a fluent-bit source tree and loaded with
 * flb_plugin_load_router; this host links the reference engine library (oracle/_ref/engine) and is built with -rdynamic, so that the
 * plugin's call of in_emitter_add_record binds to the function below instead of the engine's: it records (tag, bytes) and, for the
 * record indices it was told, answers -1 like an emitter that is busy.
 *
 *   rtag_ref_host <plugin.so> <in.mp> <out.mp> <emitted.bin> <tag as hex | -> <refused indices, comma separated | -> [name=value]...
 *
 * The filter instance is created as a processor unit (the way oracle/engine/engine_host.c creates its filters), the plugin's cb_init
 * runs inside flb_processor_init, and cb_filter is called directly with the tag.  One JSON line on stdout:
 *   {"init": false}                                       the filter did not start
 *   {"init": true, "ret": <cb_filter's answer>, "out_bytes": n, "emitted": k, "refused": j}
 * out.mp holds the output buffer when the answer is FLB_FILTER_MODIFIED; emitted.bin one entry per call of the emitter:
 *   u32 tag length, the tag, u32 size, the bytes, u8 1 when the call was answered -1 (all little endian). */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <stdint.h>
#include <fluent-bit.h>
#include <fluent-bit/flb_info.h>
#include <fluent-bit/flb_config.h>
#include <fluent-bit/flb_plugin.h>
#include <fluent-bit/flb_filter.h>
#include <fluent-bit/flb_input.h>
#include <fluent-bit/flb_processor.h>
#include <fluent-bit/flb_storage.h>

static FILE *g_emit_file;
static int g_calls, g_refusals;
static int g_refuse[256], g_nrefuse;

int in_emitter_add_record(const char *tag, int tag_len, const char *buf_data, size_t buf_size, struct flb_input_instance *in,
                          struct flb_input_instance *i_ins)
{
    uint32_t a = (uint32_t) tag_len, b = (uint32_t) buf_size;
    uint8_t refused = 0;
    int i;
    (void) in; (void) i_ins;
    for (i = 0; i < g_nrefuse; i++) if (g_refuse[i] == g_calls) refused = 1;
    fwrite(&a, 4, 1, g_emit_file);
    fwrite(tag, 1, a, g_emit_file);
    fwrite(&b, 4, 1, g_emit_file);
    fwrite(buf_data, 1, b, g_emit_file);
    fwrite(&refused, 1, 1, g_emit_file);
    g_calls++;
    g_refusals += refused;
    return refused ? -1 : 0;
}

static char *read_file(const char *path, size_t *len)
{
    FILE *f = fopen(path, "rb");
    char *b;
    long n;
    if (!f) { perror(path); exit(2); }
    fseek(f, 0, SEEK_END); n = ftell(f); fseek(f, 0, SEEK_SET);
    b = malloc(n + 1);
    if (n && fread(b, 1, n, f) != (size_t) n) { perror(path); exit(2); }
    b[n] = 0;
    fclose(f);
    *len = n;
    return b;
}

static int hexv(int c) { return c <= '9' ? c - '0' : (c | 32) - 'a' + 10; }

int main(int argc, char **argv)
{
    struct flb_config *config;
    struct flb_processor *proc;
    struct flb_processor_unit *pu;
    struct flb_filter_instance *f_ins;
    char *in, *tag;
    size_t in_len, tag_len = 0, i;
    void *out_buf = NULL;
    size_t out_size = 0;
    int ret, k;
    FILE *fo;

    if (argc < 7) { fprintf(stderr, "usage: rtag_ref_host <plugin.so> <in.mp> <out.mp> <emitted.bin> <tag hex|-> <refused|-> [name=value]...\n"); return 2; }
    tag = malloc(strlen(argv[5]) / 2 + 1);
    if (strcmp(argv[5], "-")) for (i = 0; argv[5][2 * i] && argv[5][2 * i + 1]; i++) tag[tag_len++] = (char) (hexv(argv[5][2 * i]) * 16 + hexv(argv[5][2 * i + 1]));
    if (strcmp(argv[6], "-")) {
        char *s = strdup(argv[6]), *q;
        for (q = strtok(s, ","); q && g_nrefuse < 256; q = strtok(NULL, ",")) g_refuse[g_nrefuse++] = atoi(q);
    }
    g_emit_file = fopen(argv[4], "wb");
    if (!g_emit_file) { perror(argv[4]); return 2; }

    flb_init_env();
    config = flb_config_init();
    if (!config) return 1;
    /* what flb_engine_start would have set up before any filter starts: the emitter instance cb_init creates wants an event loop for
     * its channels and config->cio for its storage */
    config->evl = mk_event_loop_create(256);
    if (!config->evl || flb_storage_create(config) != 0) { fprintf(stderr, "event loop / storage set-up failed\n"); return 1; }
    if (flb_plugin_load_router(argv[1], config) != 0) { fprintf(stderr, "flb_plugin_load_router(%s) failed\n", argv[1]); return 3; }
    proc = flb_processor_create(config, "rtag_ref_host", NULL, 0);
    if (!proc) return 1;
    pu = flb_processor_unit_create(proc, FLB_PROCESSOR_LOGS, "rewrite_tag");
    if (!pu) { fprintf(stderr, "flb_processor_unit_create(rewrite_tag) failed\n"); return 3; }
    for (k = 7; k < argc; k++) {
        char *kv = strdup(argv[k]), *eq = strchr(kv, '=');
        if (!eq) { fprintf(stderr, "bad property %s\n", argv[k]); return 2; }
        *eq = 0;
        if (flb_processor_unit_set_property_str(pu, kv, eq + 1) != 0) { printf("{\"init\": false, \"property\": \"%s\"}\n", kv); return 0; }
        free(kv);
    }
    if (flb_processor_init(proc) != 0) { printf("{\"init\": false}\n"); return 0; }
    f_ins = pu->ctx;
    in = read_file(argv[2], &in_len);
    ret = f_ins->p->cb_filter(in, in_len, tag, (int) tag_len, &out_buf, &out_size, f_ins, NULL, f_ins->context, config);
    fclose(g_emit_file);
    fo = fopen(argv[3], "wb");
    if (!fo) { perror(argv[3]); return 2; }
    if (ret == FLB_FILTER_MODIFIED && out_buf && out_size) fwrite(out_buf, 1, out_size, fo);
    fclose(fo);
    printf("{\"init\": true, \"ret\": %d, \"out_bytes\": %zu, \"emitted\": %d, \"refused\": %d}\n", ret, ret == FLB_FILTER_MODIFIED ? out_size : (size_t) 0,
           g_calls - g_refusals, g_refusals);
    fflush(stdout);
    return 0;
}
