/* tools/checklist_ref_host.c -- DEVELOPMENT-MACHINE TOOL of tools/gen_checklist_golden.py.  Drives the reference's own filter_checklist
 * on one chunk and records cb_filter's answer.  The plugin and src/flb_sqldb.c are compiled where they lie in a fluent-bit source
 * tree, against that tree's sqlite3.h, into one loadable flb-filter_checklist.so that links the machine's libsqlite3; this host loads
 * it with flb_plugin_load_router and links the reference engine library (oracle/_ref/engine).
 *
 *   checklist_ref_host <plugin.so> <in.mp> <out.mp> [name=value]...
 *
 * The engine of oracle/build_engine.sh is built with FLB_SQLDB=Off, so its struct flb_config has no sqldb_list, the one field
 * flb_sqldb_open touches.  The plugin, flb_sqldb.c and this host are therefore all compiled with -DFLB_HAVE_SQLDB: in their view the
 * list head lies over the engine's stream_processor_file / stream_processor_ctx, two pointers nothing reads in a process that never
 * starts the engine, and this host initialises it before the filter starts.  Every field behind it is shifted in this file's view,
 * so this file touches no other field of the config.
 *
 * The filter instance is created as a processor unit (the way oracle/engine/engine_host.c creates its filters), the plugin's cb_init
 * runs inside flb_processor_init, and cb_filter is called directly.  One JSON line on stdout:
 *   {"init": false}                          the filter did not start (a property the config map refuses)
 *   {"init": true, "ret": <cb_filter's answer>, "out_bytes": n, "filter_ns": <the time of the cb_filter call alone>}
 * out.mp holds the output buffer when the answer is FLB_FILTER_MODIFIED. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <stdint.h>
#include <time.h>
#include <fluent-bit.h>
#include <fluent-bit/flb_info.h>
#include <fluent-bit/flb_config.h>
#include <fluent-bit/flb_plugin.h>
#include <fluent-bit/flb_filter.h>
#include <fluent-bit/flb_input.h>
#include <fluent-bit/flb_processor.h>

#ifndef FLB_HAVE_SQLDB
#error "compile with -DFLB_HAVE_SQLDB (see the header of this file)"
#endif

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

int main(int argc, char **argv)
{
    struct flb_config *config;
    struct flb_processor *proc;
    struct flb_processor_unit *pu;
    struct flb_filter_instance *f_ins;
    char *in;
    size_t in_len;
    void *out_buf = NULL;
    size_t out_size = 0;
    int ret, k;
    FILE *fo;
    struct timespec t0, t1;

    if (argc < 4) { fprintf(stderr, "usage: checklist_ref_host <plugin.so> <in.mp> <out.mp> [name=value]...\n"); return 2; }
    flb_init_env();
    config = flb_config_init();
    if (!config) return 1;
    mk_list_init(&config->sqldb_list);
    if (flb_plugin_load_router(argv[1], config) != 0) { fprintf(stderr, "flb_plugin_load_router(%s) failed\n", argv[1]); return 3; }
    proc = flb_processor_create(config, "checklist_ref_host", NULL, 0);
    if (!proc) return 1;
    pu = flb_processor_unit_create(proc, FLB_PROCESSOR_LOGS, "checklist");
    if (!pu) { fprintf(stderr, "flb_processor_unit_create(checklist) failed\n"); return 3; }
    for (k = 4; k < argc; k++) {
        char *kv = strdup(argv[k]), *eq = strchr(kv, '=');
        if (!eq) { fprintf(stderr, "bad property %s\n", argv[k]); return 2; }
        *eq = 0;
        if (flb_processor_unit_set_property_str(pu, kv, eq + 1) != 0) { printf("{\"init\": false, \"property\": \"%s\"}\n", kv); return 0; }
        free(kv);
    }
    if (flb_processor_init(proc) != 0) { printf("{\"init\": false}\n"); return 0; }
    f_ins = pu->ctx;
    in = read_file(argv[2], &in_len);
    clock_gettime(CLOCK_MONOTONIC, &t0);
    ret = f_ins->p->cb_filter(in, in_len, "t", 1, &out_buf, &out_size, f_ins, NULL, f_ins->context, config);
    clock_gettime(CLOCK_MONOTONIC, &t1);
    fo = fopen(argv[3], "wb");
    if (!fo) { perror(argv[3]); return 2; }
    if (ret == FLB_FILTER_MODIFIED && out_buf && out_size) fwrite(out_buf, 1, out_size, fo);
    fclose(fo);
    printf("{\"init\": true, \"ret\": %d, \"out_bytes\": %zu, \"filter_ns\": %lld}\n", ret, ret == FLB_FILTER_MODIFIED ? out_size : (size_t) 0,
           (long long) (t1.tv_sec - t0.tv_sec) * 1000000000LL + (t1.tv_nsec - t0.tv_nsec));
    fflush(stdout);
    return 0;
}
