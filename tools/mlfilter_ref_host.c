/* tools/mlfilter_ref_host.c -- DEVELOPMENT-MACHINE TOOL of tools/gen_mlfilter_golden.py.  Drives the reference's own filter_multiline
 * (mode parser, buffer off) over several consecutive chunks of one filter instance.  The plugin is compiled where it lies in a
 * fluent-bit source tree and loaded with flb_plugin_load_router; this host links the reference engine library (oracle/_ref/engine).
 *
 *   mlfilter_ref_host <plugin.so> <dir> <calls> <multiline_buffer_limit | -> [P:name:type:negate:match as hex]
 *                     [R:parser:from_states:to_state:regex as hex]... [name=value]...
 *
 * P defines a [MULTILINE_PARSER] through the reference's flb_ml_parser_create (type regex / endswith / equal), R adds a rule to it
 * through flb_ml_rule_create; the parsers are initialised before the filter starts.  <dir>/in_<i>.mp are the chunks, <dir>/out_<i>.mp
 * receives the output of call i when the answer is FLB_FILTER_MODIFIED.  One JSON line on stdout:
 *   {"init": false}                      the filter did not start
 *   {"init": true, "rets": [...]}        cb_filter's answers
 * The filter instance is a processor unit (as oracle/engine/engine_host.c creates its filters); cb_filter is called directly with an
 * input instance of this host's own, because the plugin answers NOTOUCH for records of its emitter -- which is NULL with buffer off. */
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
#include <fluent-bit/multiline/flb_ml.h>
#include <fluent-bit/multiline/flb_ml_parser.h>
#include <fluent-bit/multiline/flb_ml_rule.h>

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
static char *unhex(const char *h)
{
    size_t n = strlen(h) / 2, i;
    char *o = malloc(n + 1);
    for (i = 0; i < n; i++) o[i] = (char) (hexv(h[2 * i]) * 16 + hexv(h[2 * i + 1]));
    o[n] = 0;
    return o;
}

/* "a:b:c:d" -> fields (in place) */
static int split(char *s, char **f, int max)
{
    int n = 0;
    f[n++] = s;
    for (; *s && n < max; s++) if (*s == ':') { *s = 0; f[n++] = s + 1; }
    return n;
}

#define MAXP 8
static struct { char *name; struct flb_ml_parser *p; } g_parsers[MAXP];
static int g_np;

int main(int argc, char **argv)
{
    struct flb_config *config;
    struct flb_processor *proc;
    struct flb_processor_unit *pu;
    struct flb_filter_instance *f_ins;
    struct flb_input_instance *i_ins;
    int calls, k, i, ret;
    char path[4096];

    if (argc < 5) { fprintf(stderr, "usage: mlfilter_ref_host <plugin.so> <dir> <calls> <limit|-> [P:...] [R:...] [name=value]...\n"); return 2; }
    calls = atoi(argv[3]);
    flb_init_env();
    config = flb_config_init();
    if (!config) return 1;
    config->evl = mk_event_loop_create(256);
    if (!config->evl || flb_storage_create(config) != 0) { fprintf(stderr, "event loop / storage set-up failed\n"); return 1; }
    if (strcmp(argv[4], "-")) {
        if (config->multiline_buffer_limit) flb_free(config->multiline_buffer_limit);
        config->multiline_buffer_limit = flb_strdup(argv[4]);
    }
    if (flb_plugin_load_router(argv[1], config) != 0) { fprintf(stderr, "flb_plugin_load_router(%s) failed\n", argv[1]); return 3; }
    for (k = 5; k < argc; k++) {
        char *a = strdup(argv[k]), *f[5];
        if (!strncmp(a, "P:", 2)) {
            int type;
            if (split(a, f, 5) != 5 || g_np >= MAXP) { fprintf(stderr, "bad parser %s\n", argv[k]); return 2; }
            type = !strcmp(f[2], "regex") ? FLB_ML_REGEX : !strcmp(f[2], "endswith") ? FLB_ML_ENDSWITH : FLB_ML_EQ;
            g_parsers[g_np].name = f[1];
            g_parsers[g_np].p = flb_ml_parser_create(config, f[1], type, type == FLB_ML_REGEX ? NULL : unhex(f[4]), atoi(f[3]), 1000, NULL, NULL, NULL, NULL, NULL);
            if (!g_parsers[g_np].p) { printf("{\"init\": false, \"parser\": \"%s\"}\n", f[1]); return 0; }
            g_np++;
        }
        else if (!strncmp(a, "R:", 2)) {
            if (split(a, f, 5) != 5) { fprintf(stderr, "bad rule %s\n", argv[k]); return 2; }
            for (i = 0; i < g_np; i++) if (!strcmp(g_parsers[i].name, f[1])) break;
            if (i == g_np) { fprintf(stderr, "rule for an unknown parser %s\n", f[1]); return 2; }
            if (flb_ml_rule_create(g_parsers[i].p, f[2], unhex(f[4]), f[3][0] ? f[3] : NULL, NULL) != 0) { printf("{\"init\": false, \"rule\": \"%s\"}\n", f[1]); return 0; }
        }
    }
    for (i = 0; i < g_np; i++) if (flb_ml_parser_init(g_parsers[i].p) != 0) { printf("{\"init\": false, \"parser_init\": \"%s\"}\n", g_parsers[i].name); return 0; }
    proc = flb_processor_create(config, "mlfilter_ref_host", NULL, 0);
    if (!proc) return 1;
    pu = flb_processor_unit_create(proc, FLB_PROCESSOR_LOGS, "multiline");
    if (!pu) { fprintf(stderr, "flb_processor_unit_create(multiline) failed\n"); return 3; }
    for (k = 5; k < argc; k++) {
        char *kv, *eq;
        if (!strncmp(argv[k], "P:", 2) || !strncmp(argv[k], "R:", 2)) continue;
        kv = strdup(argv[k]); eq = strchr(kv, '=');
        if (!eq) { fprintf(stderr, "bad property %s\n", argv[k]); return 2; }
        *eq = 0;
        if (flb_processor_unit_set_property_str(pu, kv, eq + 1) != 0) { printf("{\"init\": false, \"property\": \"%s\"}\n", kv); return 0; }
        free(kv);
    }
    if (flb_processor_init(proc) != 0) { printf("{\"init\": false}\n"); return 0; }
    f_ins = pu->ctx;
    i_ins = calloc(1, sizeof(*i_ins));
    snprintf(i_ins->name, sizeof(i_ins->name), "host.0");
    printf("{\"init\": true, \"rets\": [");
    for (i = 0; i < calls; i++) {
        size_t in_len, out_size = 0;
        void *out_buf = NULL;
        char *in;
        FILE *fo;
        snprintf(path, sizeof(path), "%s/in_%d.mp", argv[2], i);
        in = read_file(path, &in_len);
        ret = f_ins->p->cb_filter(in, in_len, "ml", 2, &out_buf, &out_size, f_ins, i_ins, f_ins->context, config);
        snprintf(path, sizeof(path), "%s/out_%d.mp", argv[2], i);
        fo = fopen(path, "wb");
        if (!fo) { perror(path); return 2; }
        if (ret == FLB_FILTER_MODIFIED && out_buf && out_size) fwrite(out_buf, 1, out_size, fo);
        fclose(fo);
        printf("%s%d", i ? ", " : "", ret);
        free(in);
    }
    printf("]}\n");
    fflush(stdout);
    return 0;
}
